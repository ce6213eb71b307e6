// Fused ResBlock (c1, c2) pair on ONE Winograd F(4,3) tap group for the wide k = 3 stages (C = 64 / 128; round 26):
//
//     y = x + c2( silu( c1( silu(x) ) ) )          (one iteration of ResBlock1.forward,
//                                                    fish_vocoder/modules/generators/hifigan.py:102-107)
//
// in ONE launch with 6 matrix products per FOUR outputs and (c_out, c_in) in both convs — pair_wino32_kernel's F(2,3) group leaves 8.  Same data
// flow as pair_wino32_kernel (window -> LDS once, c1's output never leaves LDS, v_mfma_f32_32x32x2_f32, waves stacked along M, weights straight
// from L2 in fragment order), on conv_wino4_impl.h's quad lattice and transform:
//   quad column n = q D + r <-> u0(n) = 4 D q + r, outputs u0 + j D (j = 0..3); X_j[n] = x'[u0(n) + j D], x4 = X0[n + D], x5 = X1[n + D];
//   points 0, +-1, +-2, inf (planes 0..5):
//     V0 = 4 x0 - 5 x2 + x4        V1 / V2 = (x4 - 4 x2) +- (x3 - 4 x1)        V3 / V4 = (x4 - x2) +- 2 (x3 - x1)        V5 = 4 x1 - 5 x3 + x5
//     U  = g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6, g0 / 24 - g1 / 12 + g2 / 6, g2   (host: pack_pair_wino4)
//     y0 = m0 + (m1 + m2) + (m3 + m4)    y1 = (m1 - m2) + 2 (m3 - m4)    y2 = (m1 + m2) + 4 (m3 + m4)    y3 = (m1 - m2) + 8 (m3 - m4) + m5
//   (the bias rides in plane 1 with weight 1: m1's coefficient is 1 in all four outputs)
// One workgroup = 4 wavefronts = WM m-tiles of 32 rows (all C rows) x WN n-tiles of 32 quad columns; a wave owns ONE (m-tile, n-tile): six accumulator
// planes of sixteen registers.
//   phase 0   silu(x) window -> LDS as X0..X3 planes of c1's lattice (all C channels)
//   per conv  for each chunk of 8 channels: X planes -> six V planes (LDS -> LDS, 12 FMA-class instructions per lattice element), barrier, MFMA
//             loop over the chunk's six fragments, barrier
//   c1 epilogue   output transform, SiLU -> X0..X3 of c2's lattice (overlaying c1's); the two columns past c1's last output are zeroed
//   c2 epilogue   output transform, + raw x (re-read from global memory: the lines phase 0 staged, requested before c2's matrix loop), 8-byte stores
// LDS: C x 4 planes of the window + one V buffer = 80.7 KB at every instance — two workgroups per CU.
#pragma once
#include "pair_wino44_impl.h"

namespace fv {

template <int DIL, int C>
struct PQ3Geom {
    static_assert(C == 64 || C == 128, "one 32-row m-tile per wave");
    static constexpr int KSZ = 3, DILV = DIL;
    static constexpr int WM = C / 32, WN = 4 / WM;
    static constexpr int CH = 8, NCHK = C / CH, NV = 6;
    static constexpr int NBQ = 32 * WN;                  // quad columns per workgroup
    static constexpr int NU = NBQ / DIL * DIL;           // ... of whole 4 D-sample blocks (the live ones)
    static constexpr int W1 = 4 * NU, TT = W1 - 2;
    static constexpr int H1 = DIL, H2 = 1, HP = H1 + H2;
    static constexpr int NQ1 = NU / DIL + 1;             // 4 D-sample blocks staged: a live column n reads X0 / X1 at n + D
    static constexpr int NP1 = 4 * DIL * NQ1;            // staged positions per channel row
    static constexpr int PX = (DIL * NQ1 + 1) / 2 * 2;   // X plane stride
    static constexpr int SX = 4 * PX;                    // channel row of the X planes: X0 X1 X2 X3
    static constexpr int PV = NBQ + 4;                   // V row stride (a 32-lane group of the MFMA read / the transform covers one row)
    static constexpr int PS = CH * PV;                   // V plane stride
    static constexpr int X_F = C * SX, V_F = NV * PS;
    // (pq_stage_window's optional raw tile: absent here)
    static constexpr bool XRES = false;
    static constexpr int XS = 0, XR_OFF = X_F + V_F;
    static constexpr int TRASH = X_F + V_F;              // one float nobody reads
    static constexpr int LDS_FLOATS = TRASH + 4;
    static constexpr int DA = 5, RA = 6;                 // weight ring: RA == the fragments of a chunk, every chunk starts at slot 0
    static_assert(PX >= NU + DIL && PX >= NBQ + 1 && PV >= NBQ, "plane strides cover both convs");
    static_assert(NP1 >= W1 + 2 * DIL, "the staged window covers c1's inputs");
    static_assert(2 * LDS_FLOATS * 4 <= 160 * 1024, "two workgroups per CU");
};

// X planes of the chunk's 8 channel rows -> six V planes [plane][channel][column]; 32 threads per channel row, consecutive columns
template <class G, int DX>
__device__ __forceinline__ void pq3_transform(const float* __restrict__ xr, float* __restrict__ v, int tid) {
    constexpr int TPR = 256 / G::CH, SLOTS = G::NBQ / TPR;
    static_assert(G::NBQ % TPR == 0, "whole slots");
    const int row = tid / TPR, c0 = tid % TPR;
    const float* xp = xr + row * G::SX + c0;
    float* dp = v + row * G::PV + c0;
    float a[SLOTS][6];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        a[j][0] = xp[TPR * j];
        a[j][1] = xp[G::PX + TPR * j];
        a[j][2] = xp[2 * G::PX + TPR * j];
        a[j][3] = xp[3 * G::PX + TPR * j];
        a[j][4] = xp[TPR * j + DX];
        a[j][5] = xp[G::PX + TPR * j + DX];
    }
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const float x0 = a[j][0], x1 = a[j][1], x2 = a[j][2], x3 = a[j][3], x4 = a[j][4], x5 = a[j][5];
        const float e4 = fmaf(-4.0f, x2, x4), o4 = fmaf(-4.0f, x1, x3), e1 = x4 - x2, o1 = x3 - x1;
        dp[TPR * j] = fmaf(4.0f, x0, fmaf(-5.0f, x2, x4));
        dp[G::PS + TPR * j] = e4 + o4;
        dp[2 * G::PS + TPR * j] = e4 - o4;
        dp[3 * G::PS + TPR * j] = fmaf(2.0f, o1, e1);
        dp[4 * G::PS + TPR * j] = fmaf(-2.0f, o1, e1);
        dp[5 * G::PS + TPR * j] = fmaf(4.0f, x1, fmaf(-5.0f, x3, x5));
    }
}

// MFMA loop over one 8-channel chunk: fragment v = plane v, four 32x32x2 MFMAs (channel pairs 0..3).  vl: the lane's base into the V planes (k-half row
// and quad column folded in).  aq: weight ring, the chunk's fragments 0 .. DA - 1 on entry, the next chunk's on exit.
template <class G>
__device__ __forceinline__ void pq3_gemm_chunk(f32x16 (&acc)[6], const float* __restrict__ vl, const __amdgpu_buffer_rsrc_t wrs, int wvoff, int wsoff,
                                               float4 (&aq)[G::RA]) {
    constexpr int DA = G::DA, RA = G::RA, NV = G::NV;
    float b_cur[4], b_nxt[4];
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) b_cur[pp] = vl[2 * pp * G::PV];
    static_for<NV>([&](auto f_c) __attribute__((always_inline)) {
        constexpr int f = decltype(f_c)::value;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 a4 = aq[f % RA];
            float apin = m == 0 ? a4.x : m == 1 ? a4.y : m == 2 ? a4.z : a4.w;
            asm volatile("" : "+v"(apin));   // (pins the MFMA between the memory operations around it: pw_gemm_chunk)
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(apin, b_cur[m], acc[f], 0, 0, 0);
            asm volatile("" : "+v"(acc[f]));
            if (m == 0) {   // the fragment DA ahead (past the conv's last one: the next m-tile's, or the zero padding of the packed weights)
                const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(wrs, wvoff, wsoff + f * 1024, 0);
                aq[(f + DA) % RA] = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
                __builtin_amdgcn_sched_barrier(0);
            }
            if (f + 1 < NV) {
                b_nxt[m] = vl[(f + 1) * G::PS + 2 * m * G::PV];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (f + 1 < NV) {
#pragma unroll
            for (int i = 0; i < 4; ++i) b_cur[i] = b_nxt[i];
        }
    });
}

__device__ __forceinline__ void pq3_output_transform(const f32x16 (&m)[6], f32x16 (&y)[4]) {
    const f32x16 s1 = m[1] + m[2], d1 = m[1] - m[2], s2 = m[3] + m[4], d2 = m[3] - m[4];
    y[0] = (m[0] + s1) + s2;
    y[1] = d1 + 2.0f * d2;
    y[2] = s1 + 4.0f * s2;
    y[3] = (d1 + 8.0f * d2) + m[5];
}

template <int DIL, int C>
__global__ __launch_bounds__(256, 2) void pair_wino4_kernel(const PairParams p) {
    using G = PQ3Geom<DIL, C>;
    constexpr int DA = G::DA, NCHK = G::NCHK, WN = G::WN;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* X = lds;
    float* V = lds + G::X_F;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lid = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);   // a clip's tiles on one XCD
    if (lid >= p.n_tiles * p.batch) return;
    const int tile = lid % p.n_tiles, b = lid / p.n_tiles;
    const int t0 = tile * G::TT;
    const int T = p.T;
    const float* __restrict__ xb = p.x + (long long)b * C * T;

    // this wave's m-tile of the packed weights: fragments [wm * NCHK * 6, (wm + 1) * NCHK * 6)
    const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w1, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, 0x7fffffff, 0x00020000);
    const int wvoff = lane * 16;
    const int wbase = __builtin_amdgcn_readfirstlane(wm * (NCHK * G::NV * 1024));
    float4 aq[G::RA];
    auto load_w = [&](const __amdgpu_buffer_rsrc_t rs, int f) __attribute__((always_inline)) {
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, wvoff, wbase + f * 1024, 0);
        return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
    };
#pragma unroll
    for (int d = 0; d < DA; ++d) aq[d] = load_w(w1rs, d);

    pq_stage_window<G, C>(xb, T, t0, wave, lane, lds);

    // C / D layout of 32x32x2: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int khalf = lane >> 5;
    const int ncol = 32 * wn + (lane & 31);   // this lane's quad column
    const int mrow0 = 32 * wm + 4 * khalf;
    f32x16 acc[6];
    auto init_acc = [&](const float* __restrict__ bias) __attribute__((always_inline)) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const f32x4w bv = *(const f32x4w*)(bias + mrow0 + 8 * rq);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[a][4 * rq + rr] = a == 1 ? bv[rr] : 0.f;
            }
        }
    };
    init_acc(p.b1);
    const float* vl = V + khalf * G::PV + ncol;
    __syncthreads();

    // ---- c1 ----
    for (int c = 0; c < NCHK; ++c) {
        pq3_transform<G, DIL>(X + c * G::CH * G::SX, V, tid);
        __syncthreads();
        pq3_gemm_chunk<G>(acc, vl, w1rs, wvoff, __builtin_amdgcn_readfirstlane(wbase + (c * G::NV + DA) * 1024), aq);
        __syncthreads();   // the V buffer (next transform) and the X planes (c1 epilogue) are free again
    }
    // c2's first weight fragments travel while the epilogue runs (the ring holds c1's overrun fragments, never used)
#pragma unroll
    for (int d = 0; d < DA; ++d) aq[d] = load_w(w2rs, d);

    // ---- c1 epilogue: silu(c1 + b1) -> X planes of c2's lattice (mid[u], u = position - (t0 - H2): X_{u & 3}[u >> 2]) ----
    {
        f32x16 y[4];
        pq3_output_transform(acc, y);
        const int q = ncol / DIL, r = ncol - q * DIL;
        const int u0 = 4 * DIL * q + r;
        const int ts = t0 - G::H2;
        const bool live = ncol < G::NU;       // (columns of a partial 4 D block produce nothing c2 reads)
        const bool edge = ts < 0 || ts + G::W1 > T;   // wave-uniform: only a row's first / last tiles zero positions outside [0, T)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = u0 + j * DIL;
            const float kin = (!edge || (ts + u >= 0 && ts + u < T)) ? 1.f : 0.f;   // zero outside [0, T): c2's zero padding
            float* w = X + mrow0 * G::SX + (u & 3) * G::PX + (u >> 2);
            if (live) {
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    float s = pw_silu(y[j][rg]);
                    if (edge) s *= kin;
                    w[((rg & 3) + 8 * (rg >> 2)) * G::SX] = s;
                }
            }
        }
        // mid[W1], mid[W1 + 1] — what the tile's last quad reads for its two outputs past TT — are not computed here: zeros, so that the quad's two kept
        // outputs see exact zeros instead of c1's stale window in their (cancelling) terms
        if (tid < 2 * C) X[(tid >> 1) * G::SX + (tid & 1) * G::PX + G::NU] = 0.f;
    }
    init_acc(p.b2);

    // the last epilogue's residual operand is requested now, from the lines phase 0 staged: its latency runs under c2's matrix loop
    const int tl = 4 * ncol;
    const int t = t0 + tl;
    const bool pair8 = (T & 1) == 0 && (((unsigned long long)p.y | (unsigned long long)p.x) & 7ull) == 0;
    unsigned va[2], vb[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {              // outputs (0, 1) and (2, 3)
        const int tlh = tl + 2 * hh;
        const bool ok0 = tlh < G::TT && t + 2 * hh < T, ok1 = tlh + 1 < G::TT && t + 2 * hh + 1 < T;
        va[hh] = ok0 ? (unsigned)(mrow0 * T + t + 2 * hh) * 4u : 0xFFFFFFFFu;
        vb[hh] = ok1 ? (unsigned)(mrow0 * T + t + 2 * hh + 1) * 4u : 0xFFFFFFFFu;
    }
    float ra[2][16], rb[2][16];
    {
        const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, (unsigned)(C * T) * 4u, 0x00020000);
        if (pair8) {   // (an even T, TT and t0: both samples of a half are inside the tile and the clip, or outside)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(xrs, va[hh], __builtin_amdgcn_readfirstlane(((rg & 3) + 8 * (rg >> 2)) * T * 4), 0);
                    ra[hh][rg] = __uint_as_float(v.x);
                    rb[hh][rg] = __uint_as_float(v.y);
                }
        } else {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const int so = __builtin_amdgcn_readfirstlane(((rg & 3) + 8 * (rg >> 2)) * T * 4);
                    ra[hh][rg] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrs, va[hh], so, 0));
                    rb[hh][rg] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrs, vb[hh], so, 0));
                }
        }
    }
    __syncthreads();

    // ---- c2 (dilation 1) ----
    for (int c = 0; c < NCHK; ++c) {
        pq3_transform<G, 1>(X + c * G::CH * G::SX, V, tid);
        __syncthreads();
        pq3_gemm_chunk<G>(acc, vl, w2rs, wvoff, __builtin_amdgcn_readfirstlane(wbase + (c * G::NV + DA) * 1024), aq);
        if (c + 1 < NCHK) __syncthreads();
    }

    // ---- c2 epilogue: + raw x -> y; the lane's four outputs are consecutive samples, stored as two 8-byte halves ----
    {
        f32x16 y[4];
        pq3_output_transform(acc, y);
        const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y + (long long)b * C * T), 0, (unsigned)(C * T) * 4u, 0x00020000);
        const bool accum = p.out_mode == OUT_ACCUM;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            float o0[16], o1[16];
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                o0[rg] = y[2 * hh][rg] + ra[hh][rg];
                o1[rg] = y[2 * hh + 1][rg] + rb[hh][rg];
            }
            if (accum) {
                float a0[16], a1[16];
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const int so = __builtin_amdgcn_readfirstlane(((rg & 3) + 8 * (rg >> 2)) * T * 4);
                    a0[rg] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yrs, va[hh], so, 0));
                    a1[rg] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yrs, vb[hh], so, 0));
                }
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    o0[rg] = (a0[rg] + o0[rg]) * p.out_scale;
                    o1[rg] = (a1[rg] + o1[rg]) * p.out_scale;
                }
            }
            if (pair8) {
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    u32x2 v;
                    v.x = __float_as_uint(o0[rg]);
                    v.y = __float_as_uint(o1[rg]);
                    __builtin_amdgcn_raw_buffer_store_b64(v, yrs, va[hh], __builtin_amdgcn_readfirstlane(((rg & 3) + 8 * (rg >> 2)) * T * 4), 0);
                }
            } else {
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const int so = __builtin_amdgcn_readfirstlane(((rg & 3) + 8 * (rg >> 2)) * T * 4);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o0[rg]), yrs, va[hh], so, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o1[rg]), yrs, vb[hh], so, 0);
                }
            }
        }
    }
}

template <int DIL, int C>
inline bool launch_pair_wino4_one(const PairParams& p, int batch, hipStream_t s) {
    using G = PQ3Geom<DIL, C>;
    static_assert(G::TT == pair_wino4_tile(DIL, C), "the profiler's grid figure");
    PairParams q = p;
    q.n_tiles = (p.T + G::TT - 1) / G::TT;
    q.batch = batch;
    const size_t lds = (size_t)G::LDS_FLOATS * sizeof(float);
    if (!FV_ENSURE_DYN_LDS((pair_wino4_kernel<DIL, C>), lds)) return false;
    hipLaunchKernelGGL((pair_wino4_kernel<DIL, C>), dim3((batch * q.n_tiles + 7) / 8 * 8), dim3(256), lds, s, q);
    return true;
}

}  // namespace fv
