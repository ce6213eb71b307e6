// Winograd F(4,3) fused (c1, c2) pair kernels of the wide stages, k = 3 (C = 64 / 128)
#include "pair_wino4_impl.h"
namespace fv {
bool launch_pair_wino4_k3(const PairParams& p, int C, int dil, int batch, hipStream_t s) {
#define FV_PQ3_CASE(D)                                                     \
    if (dil == D) {                                                        \
        if (C == 64) return launch_pair_wino4_one<D, 64>(p, batch, s);     \
        if (C == 128) return launch_pair_wino4_one<D, 128>(p, batch, s);   \
        return false;                                                      \
    }
    FV_PQ3_CASE(1) FV_PQ3_CASE(3) FV_PQ3_CASE(5)
#undef FV_PQ3_CASE
    return false;
}
}  // namespace fv
