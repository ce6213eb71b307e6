// Weight layouts of the fused conv layer (conv_pack.h): every transform in double, every layout one function.  Host code only.
#include <algorithm>
#include <cmath>

#include "conv_pack.h"

namespace fv {

// polyphase: row (co, r), taps j' = 0..ks'-1 reading x[q + j' - (ks'-1)]; torch weight is (C_in, C_out, k)
std::vector<float> polyphase_rows(const float* host_w, int c_in, int c_out, int k, int stride) {
    const int u = stride;
    const int ksp = (k + u - 1) / u;
    std::vector<float> wc((size_t)c_out * u * c_in * ksp, 0.f);
    for (int co = 0; co < c_out; ++co)
        for (int r = 0; r < u; ++r) {
            const int m = co * u + r;
            for (int ci = 0; ci < c_in; ++ci)
                for (int jp = 0; jp < ksp; ++jp) {
                    const int tap = r + (ksp - 1 - jp) * u;
                    if (tap < k) wc[((size_t)m * c_in + ci) * ksp + jp] = host_w[((size_t)ci * c_out + co) * k + tap];
                }
        }
    return wc;
}

// Packed layout (float4 units):  [(m_tile * nchunk + chunk) * ks + tap] * 64 + lane
//   .{x,y,z,w}[pp] = Wc[m_tile*32 + (lane & 31)][chunk*8 + 2*pp + (lane >> 5)][tap]     (0 outside M x Cin)
// i.e. exactly the A fragment of v_mfma_f32_32x32x2_f32 for k-step (tap, channel pair pp): lane l supplies
// row l&31, k-half l>>5 — one coalesced 1 KiB global_load_dwordx4 per wave per tap.
std::vector<float> pack_conv_weights(const std::vector<float>& wc, int M, int Cin, int ks, int m_pad, int nchunk) {
    const int mtiles = m_pad / 32;
    // + 8 zero k-steps after the last m-tile: the kernels' weight prefetch runs a few steps past the end
    std::vector<float> out(((size_t)mtiles * nchunk * ks + 8) * 64 * 4, 0.f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int c = 0; c < nchunk; ++c)
            for (int j = 0; j < ks; ++j)
                for (int l = 0; l < 64; ++l) {
                    const int m = mt * 32 + (l & 31);
                    if (m >= M) continue;
                    float* dst = &out[((((size_t)mt * nchunk + c) * ks + j) * 64 + l) * 4];
                    for (int pp = 0; pp < 4; ++pp) {
                        const int ci = c * kChunk + 2 * pp + (l >> 5);
                        if (ci < Cin) dst[pp] = wc[((size_t)m * Cin + ci) * ks + j];
                    }
                }
    return out;
}

// Winograd F(2,3) tap groups (conv_wino_impl.h): groups at taps 0, 4, 8 -> four transformed weights each, the taps between them
// (3, 7) -> (+w, -w); virtual-tap order = WinoGeom::off_of / acc_of
std::vector<float> wino_taps(const std::vector<float>& wc, int c_out, int c_in, int k) {
    const int ng = (k + 1) / 4, ns = (k - 3) / 4;
    const int nv = wino_nv(k);
    std::vector<float> ww((size_t)c_out * c_in * nv);
    for (size_t oc = 0; oc < (size_t)c_out * c_in; ++oc) {
        const float* w = &wc[oc * k];
        float* o = &ww[oc * nv];
        for (int g = 0; g < ng; ++g) {
            const double g0 = w[4 * g], g1 = w[4 * g + 1], g2 = w[4 * g + 2];
            o[4 * g + 0] = (float)g0;
            o[4 * g + 1] = (float)((g0 + g1 + g2) * 0.5);
            o[4 * g + 2] = (float)((g0 - g1 + g2) * 0.5);
            o[4 * g + 3] = (float)g2;
        }
        for (int s2 = 0; s2 < ns; ++s2) {
            o[4 * ng + 2 * s2] = w[4 * s2 + 3];
            o[4 * ng + 2 * s2 + 1] = -w[4 * s2 + 3];
        }
    }
    return ww;
}

// Winograd F(4,3) tap groups (conv_wino4_impl.h): per (32-row tile, plane half h) nv4 = 3 ng + 2 ns virtual taps = Wino4Geom::off_of / acc_of:
// group g, i = 0..2 -> transformed weight U_p of taps 4g..4g+2 with p = i (h = 0: m0 m1 m2) or 5 - i (h = 1: m5 m4 m3); then per single tap
// 4s + 3 two plain copies (h = 0: into m0 and S1, h = 1: into m5 and S2).  Packed as 2 M rows: row (2 mt + h) * 32 + r = (row 32 mt + r, half h)
std::vector<float> wino4_rows(const std::vector<float>& wc, int c_out, int c_in, int k) {
    const int ng = (k + 1) / 4, ns = (k - 3) / 4;
    const int nv4 = wino4_nv(k);
    std::vector<float> w4((size_t)2 * c_out * c_in * nv4);
    for (int co = 0; co < c_out; ++co)
        for (int hh = 0; hh < 2; ++hh)
            for (int ci = 0; ci < c_in; ++ci) {
                const float* w = &wc[((size_t)co * c_in + ci) * k];
                float* o = &w4[((size_t)((co / 32 * 2 + hh) * 32 + co % 32) * c_in + ci) * nv4];
                for (int g = 0; g < ng; ++g) {
                    const double g0 = w[4 * g], g1 = w[4 * g + 1], g2 = w[4 * g + 2];
                    const double U[6] = {g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2};
                    for (int i = 0; i < 3; ++i) o[3 * g + i] = (float)U[hh == 0 ? i : 5 - i];
                }
                for (int s2 = 0; s2 < ns; ++s2) o[3 * ng + 2 * s2] = o[3 * ng + 2 * s2 + 1] = w[4 * s2 + 3];
            }
    return w4;
}

// F(4,4) weight transform, points ±1/2, ±1, ±2 (the ∞ plane is the group's fourth tap itself): U(plane) = sum_t G44[plane][t] * tap 4 g + t
static const double G44[6][4] = {{16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45}, {-16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45}, {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
                                 {2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},   {1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},    {-1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45}};

namespace {
struct Taps44 {   // wc (c_out, c_in, k) read as tap groups of four: taps past k and channels past c_in are zero
    const std::vector<float>& wc;
    int c_in, k;
    double tap(int co, int ci, int j) const { return (j < k && ci < c_in) ? (double)wc[((size_t)co * c_in + ci) * k + j] : 0.0; }
    float plane(int co, int ci, int g, int pl) const {
        double u = 0.0;
        for (int t = 0; t < 4; ++t) u += G44[pl][t] * tap(co, ci, 4 * g + t);
        return (float)u;
    }
};
}  // namespace

// Winograd F(4,4) tap groups (conv_wino44_impl.h): groups of FOUR taps at 0, 4, 8 (taps past k are zero), points ±1/2, ±1, ±2, ∞.  Per (32-row tile,
// plane half h) and 8-channel block: 3 ng full fragments — group g, own plane i (h = 0: +1/2, -1/2, +1; h = 1: -1, +2, -2), the four channel pairs
// in .xyzw — then ONE fragment of the shared ∞ plane (U = the group's fourth tap): component j = group j / 2, channel pair 2 h + j % 2
std::vector<float> pack_wino44(const std::vector<float>& wc, int c_out, int c_in, int k, int nchunk) {
    const int ng4 = (k + 3) / 4, nv44 = 3 * ng4 + 1, mts = c_out / 32;
    const Taps44 w{wc, c_in, k};
    std::vector<float> p44(((size_t)mts * 2 * nchunk * nv44 + 8) * 64 * 4, 0.f);
    for (int mt = 0; mt < mts; ++mt)
        for (int hh = 0; hh < 2; ++hh)
            for (int c = 0; c < nchunk; ++c)
                for (int v = 0; v < nv44; ++v)
                    for (int l = 0; l < 64; ++l) {
                        const int co = 32 * mt + (l & 31);
                        float* dst = &p44[(((((size_t)mt * 2 + hh) * nchunk + c) * nv44 + v) * 64 + l) * 4];
                        for (int j = 0; j < 4; ++j) {
                            if (v < 3 * ng4) {
                                const int g = v / 3, pl = 3 * hh + v % 3, ci = 8 * c + 2 * j + (l >> 5);
                                dst[j] = w.plane(co, ci, g, pl);
                            } else {
                                const int g = j / 2, ci = 8 * c + 2 * (2 * hh + j % 2) + (l >> 5);
                                dst[j] = g < ng4 - 1 ? (float)w.tap(co, ci, 4 * g + 3) : 0.f;
                            }
                        }
                    }
    return p44;
}

// A fragments of v_mfma_f32_16x16x4_f32 (row = lane & 15, k = lane >> 4), one float4 per lane = A operands of four MFMAs: fragment
// ((mt * nblk + blk) * nf + f), .{x,y} = virtual tap 2 f, channel quads 0 / 1 of 8-channel block blk (channels 8 blk + {0..3}, {4..7});
// .{z,w} = virtual tap 2 f + 1; + 8 zero fragments of prefetch overrun.  tap(co, ci, v): the virtual tap's value
template <class Tap>
static std::vector<float> gather_16x16x4(int mts, int nblk, int nf, Tap tap) {
    std::vector<float> out(((size_t)mts * nblk * nf + 8) * 64 * 4, 0.f);
    for (int mt = 0; mt < mts; ++mt)
        for (int blk = 0; blk < nblk; ++blk)
            for (int f = 0; f < nf; ++f)
                for (int l = 0; l < 64; ++l)
                    for (int q = 0; q < 4; ++q) {
                        const int co = 16 * mt + (l & 15), ci = 8 * blk + 4 * (q & 1) + (l >> 4), v = 2 * f + (q >> 1);
                        out[((((size_t)mt * nblk + blk) * nf + f) * 64 + l) * 4 + q] = tap(co, ci, v);
                    }
    return out;
}

// conv_wino_lat_impl.h: fragment ((mt * nblk + blk) * nv / 2 + vp) of gather_16x16x4 over the F(2,3) virtual taps ww (c_out, c_in, nv)
std::vector<float> pack_wino_lat(const std::vector<float>& ww, int c_out, int c_in, int nv) {
    return gather_16x16x4(c_out / 16, c_in / 8, nv / 2, [&](int co, int ci, int v) { return ww[((size_t)co * c_in + ci) * nv + v]; });
}

// pair_wino44_impl.h (C = 16 / 32), conv_wino_lat44_impl.h (whole 32-row blocks): F(4,4) tap groups (the G44 transform of pack_wino44) as
// gather_16x16x4 fragments.  Virtual tap v of a channel: group v / 7, plane v % 7 (+1/2 -1/2 +1 -1 +2 -2 inf; the last group has no inf tap)
std::vector<float> pack_wino44_16(const std::vector<float>& wc, int c_in, int k) {
    const int ng4 = (k + 3) / 4, nvq = 7 * (ng4 - 1) + 6, nfq = (nvq + 1) / 2;
    const Taps44 w{wc, c_in, k};
    return gather_16x16x4(c_in / 16, c_in / 8, nfq, [&](int co, int ci, int v) -> float {
        if (v >= nvq) return 0.f;
        const int g = v / 7, pl = v % 7;
        return pl == 6 ? (float)w.tap(co, ci, 4 * g + 3) : w.plane(co, ci, g, pl);
    });
}

// pair_wino_impl.h: A fragments of v_mfma_f32_16x16x4_f32 (row = lane & 15, k = lane >> 4), one float4 per lane = four MFMAs.
//   C = 16: fragment v            .{x,y,z,w}[s]       = W'[lane & 15][4 s + (lane >> 4)][v]                      (16 channels)
//   C = 32: fragment sb * nv + v  .{x,y,z,w}[2 s + mt] = W'[16 mt + (lane & 15)][8 sb + 4 s + (lane >> 4)][v]   (8 channels, both m-tiles)
// + 8 zero fragments: the kernels' weight ring runs a few fragments past the end
std::vector<float> pack_pair_wino16(const std::vector<float>& ww, int c_in, int nv) {
    const int mt_n = c_in / 16, fch = 16 / mt_n, nfr = c_in / fch * nv;
    std::vector<float> p16((size_t)(nfr + 8) * 64 * 4, 0.f);
    for (int sb = 0; sb < c_in / fch; ++sb)
        for (int v = 0; v < nv; ++v)
            for (int l = 0; l < 64; ++l)
                for (int q = 0; q < 4; ++q) {
                    const int s = mt_n == 2 ? q / 2 : q, mt = mt_n == 2 ? q % 2 : 0;
                    const int co = 16 * mt + (l & 15), ci = fch * sb + 4 * s + (l >> 4);
                    p16[(((size_t)sb * nv + v) * 64 + l) * 4 + q] = ww[((size_t)co * c_in + ci) * nv + v];
                }
    return p16;
}

// pair_wino4_impl.h (C = 64 / 128, k = 3): ONE F(4,3) tap group per (c_out, c_in), points 0, +-1, +-2, inf — wino4_rows' transform, all six planes in
// one row: U = g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2
std::vector<float> pair_wino4_taps(const std::vector<float>& wc, int c) {
    std::vector<float> u6((size_t)c * c * 6);
    for (size_t oc = 0; oc < (size_t)c * c; ++oc) {
        const double g0 = wc[oc * 3], g1 = wc[oc * 3 + 1], g2 = wc[oc * 3 + 2];
        const double U[6] = {g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2};
        for (int v = 0; v < 6; ++v) u6[oc * 6 + v] = (float)U[v];
    }
    return u6;
}

// ... in pack_conv_weights' fragment order with the six planes as taps: float4 [(m_tile * (c / 8) + chunk) * 6 + plane] * 64 + lane,
// .{x,y,z,w}[pp] = U[32 m_tile + (lane & 31)][8 chunk + 2 pp + (lane >> 5)][plane]; + 8 zero fragments of prefetch overrun
std::vector<float> pack_pair_wino4(const std::vector<float>& wc, int c) { return pack_conv_weights(pair_wino4_taps(wc, c), c, c, 6, c, c / kChunk); }

// v_mfma_f32_16x16x4_f32 A fragments: [tap][lane] float4, .q = W[lane & 15][4q + (lane >> 4)][tap]
std::vector<float> pack_conv16(const float* host_w, int k) {
    std::vector<float> p16((size_t)k * 64 * 4);
    for (int j = 0; j < k; ++j)
        for (int l = 0; l < 64; ++l)
            for (int q = 0; q < 4; ++q)
                p16[((size_t)j * 64 + l) * 4 + q] = host_w[((size_t)(l & 15) * 16 + 4 * q + (l >> 4)) * k + j];
    return p16;
}

// s_w: power of two with max|w| * s_w in [2^13, 2^14)
float f16x3_weight_scale(const float* w, size_t n) {
    float wmax = 0.f;
    for (size_t i = 0; i < n; ++i) wmax = std::max(wmax, std::fabs(w[i]));
    int e = 0;
    if (wmax > 0.f && std::isfinite(wmax)) {
        (void)std::frexp(wmax, &e);   // wmax = f * 2^e, f in [0.5, 1)
        e = 14 - e;                   // wmax * 2^e in [2^13, 2^14)
    }
    return std::ldexp(1.0f, e);
}

// f16x3 precision mode (conv_f16x3_impl.h).  Packed layout, 16-byte units (8 halfs):
//   [((m_tile * nch16 + chunk) * ks + tap) * 2 + plane] * 64 + lane,   halfs i = 0..7:
//   plane(Wc[m_tile*32 + (lane & 31)][chunk*16 + 8*(lane >> 5) + i][tap] * s_w),   planes: wh, wl = w*s_w - wh
//   (the third operand plane wh * 2^-11 is a packed multiply in registers: one third less weight traffic per MFMA)
// = the A fragment of v_mfma_f32_32x32x16_f16 for k-block (chunk, tap).  s_w: f16x3_weight_scale() of the layer's weights.
std::vector<_Float16> pack_conv_weights_f16x3(const std::vector<float>& wc, int M, int Cin, int ks, int m_pad, int nch16, float s_w) {
    const int mtiles = m_pad / 32;
    // + 4 zero k-blocks after the last m-tile: the weight prefetch runs a few blocks past the end
    std::vector<_Float16> out(((size_t)mtiles * nch16 * ks + 4) * 2 * 64 * 8, (_Float16)0.f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int c = 0; c < nch16; ++c)
            for (int j = 0; j < ks; ++j)
                for (int l = 0; l < 64; ++l) {
                    const int m = mt * 32 + (l & 31);
                    if (m >= M) continue;
                    const size_t blk = (((size_t)mt * nch16 + c) * ks + j) * 2;
                    for (int i = 0; i < 8; ++i) {
                        const int ci = c * 16 + 8 * (l >> 5) + i;
                        if (ci >= Cin) continue;
                        const float w = wc[((size_t)m * Cin + ci) * ks + j] * s_w;   // exact: power-of-two scale
                        const _Float16 wh = (_Float16)w;
                        const _Float16 wl = (_Float16)(w - (float)wh);
                        out[((blk + 0) * 64 + l) * 8 + i] = wh;
                        out[((blk + 1) * 64 + l) * 8 + i] = wl;
                    }
                }
    return out;
}

// pair16_f16x3.hip: row (s, co) of tap block jj in [0, k] holds w[co][:, jj - s] (two output samples per channel
// share one activation fragment); 32x32x16 A-fragment order, (wh, wl) planes, + 4 zero blocks of prefetch overrun
std::vector<_Float16> pack_pair16_f16x3(const float* host_w, int k, float s_w) {
    std::vector<_Float16> ph((size_t)(k + 1 + 4) * 2 * 64 * 8, (_Float16)0.f);
    for (int jj = 0; jj <= k; ++jj)
        for (int l = 0; l < 64; ++l) {
            const int s = (l & 31) >> 4, co = l & 15, j = jj - s;
            if (j < 0 || j >= k) continue;
            for (int i = 0; i < 8; ++i) {
                const int ci = 8 * (l >> 5) + i;
                const float w = host_w[((size_t)co * 16 + ci) * k + j] * s_w;   // exact: power-of-two scale
                const _Float16 wh = (_Float16)w;
                ph[(((size_t)jj * 2 + 0) * 64 + l) * 8 + i] = wh;
                ph[(((size_t)jj * 2 + 1) * 64 + l) * 8 + i] = (_Float16)(w - (float)wh);
            }
        }
    return ph;
}

}  // namespace fv
