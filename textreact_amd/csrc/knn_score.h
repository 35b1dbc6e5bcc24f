// knn_score.h -- the canonical fp64 score of one (query, corpus row) pair, shared by the kernels that re-score candidates
// (knn_select.hip: select, wide re-score, exact scan, hostile rows; knn_range.hip: the range re-score).
//
// Canonical score = oracle/flat_knn_ref.c:trxo_score_canonical (same operations, same order):
//   IP: s = fma((double)x[k], (double)y[k], s)      L2: t = (double)x[k]-(double)y[k]; s = fma(t,t,s)
// for k = 0..d-1.  fp64 fma is IEEE on gfx950 (v_fma_f64), so the bits agree with the host.
#pragma once
#include "knn_common.h"

namespace trx {

template <bool BF>
__device__ __forceinline__ double load_as_double(const void* base, int64_t off) {
    if (BF) return (double)bf16_to_f32(reinterpret_cast<const bf16_t*>(base)[off]);
    return (double)reinterpret_cast<const float*>(base)[off];
}

// canonical score of (query row q, corpus row c); one thread walks the whole row in k order.
template <bool L2, bool CBF, bool QBF>
__device__ __forceinline__ double canonical_score(const void* qrow, const void* crow, int d) {
    double s = 0.0;
    // 8 components per step: 16-byte loads for bf16 rows, 2 x 16 bytes for f32 rows -- when both rows start on a dword: a
    // multi-dword load needs that much, and bf16 rows of an odd d start on odd halfwords every other row (device bf16 queries; since
    // round 6 also every integer host array, which reaches the device as int8 and is widened to bf16 rows of d components: the fuzzer
    // found d = 65).  Otherwise component by component: the same chain in the same order, the same bits.
    int k = 0;
    const bool dword_rows = ((reinterpret_cast<uintptr_t>(qrow) | reinterpret_cast<uintptr_t>(crow)) & 3u) == 0;
    for (; dword_rows && k + 8 <= d; k += 8) {
        double x[8], y[8];
        if (QBF) {
            uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(qrow) + k);
            const u32 w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[2 * i] = (double)__uint_as_float(w[i] << 16);
                x[2 * i + 1] = (double)__uint_as_float(w[i] & 0xffff0000u);
            }
        } else {
            const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(qrow) + k);
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(qrow) + k + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        }
        if (CBF) {
            uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(crow) + k);
            const u32 w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                y[2 * i] = (double)__uint_as_float(w[i] << 16);
                y[2 * i + 1] = (double)__uint_as_float(w[i] & 0xffff0000u);
            }
        } else {
            const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(crow) + k);
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(crow) + k + 4);
            y[0] = a.x; y[1] = a.y; y[2] = a.z; y[3] = a.w; y[4] = b.x; y[5] = b.y; y[6] = b.z; y[7] = b.w;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (L2) { const double t = x[i] - y[i]; s = __builtin_fma(t, t, s); }
            else s = __builtin_fma(x[i], y[i], s);
        }
    }
    for (; k < d; ++k) {
        const double x = load_as_double<QBF>(qrow, k), y = load_as_double<CBF>(crow, k);
        if (L2) { const double t = x - y; s = __builtin_fma(t, t, s); }
        else s = __builtin_fma(x, y, s);
    }
    return s;
}

}  // namespace trx
