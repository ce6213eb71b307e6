// Weight layouts of the fused conv layer: folded torch-layout weights (host) -> the fragment orders the kernels load.
// Pure host functions: no device, no HIP runtime — conv_layer_create (conv_layer.hip) decides which forms a layer keeps and uploads them.
#pragma once

#include <cstddef>
#include <vector>

namespace fv {

constexpr int kChunk = 8;  // input channels staged per LDS chunk (= 4 MFMA k-steps of 2 per tap)

// Virtual taps per (c_out, c_in) of the Winograd forms (k in {3, 7, 11})
inline int wino_nv(int k) { return 4 * ((k + 1) / 4) + 2 * ((k - 3) / 4); }    // F(2,3): WinoGeom::off_of / acc_of
inline int wino4_nv(int k) { return 3 * ((k + 1) / 4) + 2 * ((k - 3) / 4); }   // F(4,3), per plane half: Wino4Geom::off_of / acc_of

// ConvTranspose1d -> polyphase rows (c_out * stride, c_in, ceil(k / stride)); host_w in torch layout (c_in, c_out, k)
std::vector<float> polyphase_rows(const float* host_w, int c_in, int c_out, int k, int stride);

// 32x32x2 fragment order of rows wc (M, Cin, ks)
std::vector<float> pack_conv_weights(const std::vector<float>& wc, int M, int Cin, int ks, int m_pad, int nchunk);

// Winograd forms of the C -> C ResBlock / AMPBlock convs: wc (c_out, c_in, k), k in {3, 7, 11}
std::vector<float> wino_taps(const std::vector<float>& wc, int c_out, int c_in, int k);     // F(2,3) virtual taps (c_out, c_in, wino_nv(k))
std::vector<float> wino4_rows(const std::vector<float>& wc, int c_out, int c_in, int k);    // F(4,3) rows (2 c_out, c_in, wino4_nv(k))
std::vector<float> pack_wino44(const std::vector<float>& wc, int c_out, int c_in, int k, int nchunk);   // F(4,4) quad-lattice fragments
std::vector<float> pack_wino_lat(const std::vector<float>& ww, int c_out, int c_in, int nv);            // 16x16x4 latency fragments of wino_taps()
std::vector<float> pack_wino44_16(const std::vector<float>& wc, int c_in, int k);                       // 16x16x4 F(4,4) fragments
std::vector<float> pack_pair_wino16(const std::vector<float>& ww, int c_in, int nv);                    // C = 16 / 32 pair fragments of wino_taps()
std::vector<float> pack_conv16(const float* host_w, int k);                                             // plain 16x16x4 fragments, 16 -> 16 channels
std::vector<float> pair_wino4_taps(const std::vector<float>& wc, int c);                                // k = 3, C -> C: the F(4,3) group U = G w, (c, c, 6)
std::vector<float> pack_pair_wino4(const std::vector<float>& wc, int c);                                // ... as 32x32x2 fragments (pair_wino4_impl.h)

// f16x3 precision mode: s_w, and the (wh, wl) planes of w * s_w
float f16x3_weight_scale(const float* w, size_t n);
std::vector<_Float16> pack_conv_weights_f16x3(const std::vector<float>& wc, int M, int Cin, int ks, int m_pad, int nch16, float s_w);
std::vector<_Float16> pack_pair16_f16x3(const float* host_w, int k, float s_w);

}  // namespace fv
