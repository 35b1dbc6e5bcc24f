// knn_range.hip -- the kernels of the range search (knn_range.h; host side: knn_api.hip, trx_index_range_search).
//
// Replaces the inside of faiss::IndexFlat::range_search (IndexFlatL2 / IndexFlatIP): every row with D < radius (L2) or
// D > radius (inner product), D = (float) of the canonical fp64 score, per query in ascending id.
//
// The scan kernel (knn_scan.hip) runs unchanged in its fixed-threshold mode: a query's threshold is the seed written here, and
// every row whose approximate key reaches it is listed.  The seed is the predicate's key bound lowered by twice the key error
// bound, so that no row that satisfies the predicate can stay unlisted; a list that would overflow is compacted by the scan
// (its bound rises above the seed) and the query then takes the exact fp64 scan.
#include "../../include/trx_knn.h"
#include "knn_range.h"
#include "knn_score.h"
#include <float.h>

namespace trx {

template <bool L2, bool QBF>
__global__ __launch_bounds__(256) void range_seed_kernel(const void* queries, int64_t nq, int d, double radius, const float* qnorm2, float eps_rel,
                                                         float eps_round, float ymax_norm2, const float* qerr2, float yerr2_max, float* seed,
                                                         u32* g_thr) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float xn2 = qnorm2[q];
    float sd = __builtin_inff();       // a hostile query (knn_common.h): nothing is listed, the rescore sends it to the exact path
    if (!hostile_norm2(xn2)) {
        // eps_q exactly as the select kernel's certificate computes it: a bound of |key^ - key| for every row of this query
        const float bq = L2 ? (2.0f * sqrtf(xn2 * ymax_norm2) + ymax_norm2) : sqrtf(xn2 * ymax_norm2);
        const float bx = L2 ? 2.0f * sqrtf(xn2 * ymax_norm2) : sqrtf(xn2 * ymax_norm2);
        const double eps = ((double)eps_rel * (double)bq + round_term(eps_round, bx, xn2, qerr2, q, ymax_norm2, yerr2_max, L2)) * 1.0001 + 1e-30;
        // key = 2 x.y - |y|^2 = |x|^2 - D (L2), x.y = D (IP).  (float)D < r implies D < r, and D > r likewise (round to nearest):
        // the fp64 D is the exact value up to ~d 2^-53 of its terms, far inside eps.  |x|^2 here is the fp64 sum of squares.
        double t = radius, mag = fabs(radius);
        if (L2) {
            double xx = 0.0;
            const char* qrow = reinterpret_cast<const char*>(queries) + q * (int64_t)d * (QBF ? 2 : 4);
            for (int k = 0; k < d; ++k) { const double v = load_as_double<QBF>(qrow, k); xx = __builtin_fma(v, v, xx); }
            t = xx - radius;
            mag += xx;
        }
        const double low = t - 2.0 * eps - 1e-6 * (fabs(t) + mag);
        sd = low < -(double)FLT_MAX ? -__builtin_inff() : __double2float_rd(low);      // (-inf: every row is listed -> exact path)
    }
    seed[q] = sd;
    const u32 o = ordkey(sd);
    u32* g = g_thr + (q >> 8) * 1024 + (q & 255);
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) g[sl * 256] = o;
}

hipError_t launch_range_seeds(int metric, const void* q, int is_bf, int64_t nq, int d, double radius, const float* qnorm2, float eps_rel,
                              float eps_round, float ymax_norm2, const float* qerr2, float yerr2_max, float* seed, u32* g_thr, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    dim3 grid((unsigned)((nq + 255) / 256)), block(256);
#define TRX_RS(a, b) hipLaunchKernelGGL((range_seed_kernel<a, b>), grid, block, 0, st, q, nq, d, radius, qnorm2, eps_rel, eps_round, ymax_norm2, qerr2, yerr2_max, seed, g_thr)
    if (metric) { if (is_bf) TRX_RS(true, true); else TRX_RS(true, false); }
    else { if (is_bf) TRX_RS(false, true); else TRX_RS(false, false); }
#undef TRX_RS
    return hipGetLastError();
}

// One workgroup per query (grid-stride).  T = the largest bound of the query's lists: above the packed seed only when a list was
// compacted, i.e. rows that reach the seed may be missing -> exact path.  Otherwise every listed row (pad rows of the last
// tile and the index's hostile rows left out) and every hostile row are scored, the ones whose (float) score satisfies the
// predicate kept, sorted by id in LDS and written over the query's own lists.
template <bool L2, bool CBF, bool QBF>
__global__ __launch_bounds__(256) void range_rescore_kernel(RangeParams p) {
    __shared__ u32 r_id[RANGE_LIST_MAX + MAX_SPECIAL];
    __shared__ u64 r_row[RANGE_ROWS_MAX];
    __shared__ u64 red[256];
    __shared__ int r_c, r_s;
    const int tid = threadIdx.x;
    constexpr int QE = QBF ? 2 : 4, CE = CBF ? 2 : 4;
    const int region = p.nlists * p.cap_alloc;
    for (int q = blockIdx.x; q < p.nq; q += gridDim.x) {
        __syncthreads();
        u64 t = 0ull;
        for (int l = tid; l < p.nlists; l += 256) { const u64 b = p.cand_thr[(int64_t)q * p.nlists + l]; t = b > t ? b : t; }
        red[tid] = t;
        if (tid == 0) { r_c = 0; r_s = 0; }
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w && red[tid + w] > red[tid]) red[tid] = red[tid + w]; __syncthreads(); }
        const float sd = p.seed[q];
        const u64 seedb = sd > -__builtin_inff() ? (u64)ordkey(sd) << 32 : 0ull;
        bool to_exact = red[0] > seedb || hostile_norm2(p.qnorm2[q]) || !(sd > -__builtin_inff());
        if (!to_exact) {
            for (int l = tid >> 6; l < p.nlists; l += 4) {
                const int64_t o = (int64_t)q * p.nlists + l;
                const int cnt = (int)p.cand_cnt[o];
                for (int i = tid & 63; i < cnt; i += 64) {
                    const u64 e = p.cand[o * p.cap_alloc + i];
                    const u32 id = comp_id(e);
                    if (e != 0ull && (int64_t)id < p.n && !(p.nspecial && in_sorted_ids(p.special, p.nspecial, id))) {
                        const int pos = atomicAdd(&r_c, 1);
                        if (pos < RANGE_LIST_MAX + MAX_SPECIAL) r_id[pos] = id;
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < p.nspecial; i += 256) {
                const int pos = atomicAdd(&r_c, 1);
                if (pos < RANGE_LIST_MAX + MAX_SPECIAL) r_id[pos] = (u32)p.special[i];
            }
            __syncthreads();
            const int C = min(r_c, RANGE_LIST_MAX + MAX_SPECIAL);      // (the host keeps nlists <= 32 and nspecial <= MAX_SPECIAL)
            const char* qrow = reinterpret_cast<const char*>(p.query_orig) + (int64_t)q * p.ld_q * QE;
            for (int i = tid; i < C; i += 256) {
                const u32 id = r_id[i];
                const char* crow = reinterpret_cast<const char*>(p.corpus_orig) + (int64_t)id * p.ld_c * CE;
                const float df = (float)canonical_score<L2, CBF, QBF>(qrow, crow, p.d);
                const bool keep = L2 ? df < p.radius : df > p.radius;      // (a NaN score never satisfies it)
                if (keep) {
                    const int pos = atomicAdd(&r_s, 1);
                    if (pos < RANGE_ROWS_MAX) r_row[pos] = ((u64)id << 32) | (u64)__float_as_uint(df);
                }
            }
            __syncthreads();
            const int S = r_s;
            if (S > RANGE_ROWS_MAX || S > region || r_c > RANGE_LIST_MAX + MAX_SPECIAL) to_exact = true;
            else {
                int N = 2; while (N < S) N <<= 1;
                for (int i = S + tid; i < N; i += 256) r_row[i] = ~0ull;
                __syncthreads();
                for (int size = 2; size <= N; size <<= 1) {          // bitonic, ascending (the id is the high word: id order)
                    for (int stride = size >> 1; stride > 0; stride >>= 1) {
                        for (int i = tid; i < (N >> 1); i += 256) {
                            const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                            const u64 a = r_row[lo], b = r_row[hi];
                            if ((a > b) == ((lo & size) == 0)) { r_row[lo] = b; r_row[hi] = a; }
                        }
                        __syncthreads();
                    }
                }
                u64* out = p.rows + (int64_t)q * region;
                for (int i = tid; i < S; i += 256) out[i] = r_row[i];
                if (tid == 0) { p.cnt[q] = S; p.exact[q] = 0; }
            }
        }
        if (to_exact && tid == 0) { p.cnt[q] = 0; p.exact[q] = 1; p.xlist[atomicAdd(p.nx, 1)] = q; }
    }
}

hipError_t launch_range_rescore(const RangeParams& p, hipStream_t st) {
    if (p.nq <= 0) return hipSuccess;
    dim3 grid((unsigned)(p.nq < 4096 ? p.nq : 4096)), block(256);
    const int sel = (p.metric ? 4 : 0) | (p.corpus_is_bf16 ? 2 : 0) | (p.query_is_bf16 ? 1 : 0);
#define TRX_RR(a, b, c) hipLaunchKernelGGL((range_rescore_kernel<a, b, c>), grid, block, 0, st, p)
    switch (sel) {
        case 0: TRX_RR(false, false, false); break;
        case 1: TRX_RR(false, false, true); break;
        case 2: TRX_RR(false, true, false); break;
        case 3: TRX_RR(false, true, true); break;
        case 4: TRX_RR(true, false, false); break;
        case 5: TRX_RR(true, false, true); break;
        case 6: TRX_RR(true, true, false); break;
        default: TRX_RR(true, true, true); break;
    }
#undef TRX_RR
    return hipGetLastError();
}

// exclusive scan of the counts, one workgroup: a thread sums a contiguous run, the 1,024 partial sums are scanned in LDS
__global__ __launch_bounds__(1024) void range_lims_kernel(const int* cnt, int nq, int64_t base, int64_t* lims) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int per = (nq + 1023) / 1024;
    const int a = min(nq, tid * per), b = min(nq, a + per);
    int64_t s = 0;
    for (int i = a; i < b; ++i) s += cnt[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = base + part[tid] - s;
    for (int i = a; i < b; ++i) { lims[i] = run; run += cnt[i]; }
    if (tid == 1023) lims[nq] = base + part[1023];
}

hipError_t launch_range_lims(const int* cnt, int nq, int64_t base, int64_t* lims, hipStream_t st) {
    hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(1024), 0, st, cnt, nq, base, lims);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void range_emit_kernel(const u64* rows, int region, const int* cnt, const int* exact, const int64_t* lims,
                                                         int64_t base, int nq, float* D, int64_t* I) {
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        if (exact[q]) continue;
        const int c = cnt[q];
        const int64_t o = lims[q] - base;
        const u64* src = rows + (int64_t)q * region;
        for (int i = threadIdx.x; i < c; i += 256) {
            const u64 v = src[i];
            D[o + i] = __uint_as_float((u32)v);
            I[o + i] = (int64_t)(v >> 32);
        }
    }
}

hipError_t launch_range_emit(const u64* rows, int region, const int* cnt, const int* exact, const int64_t* lims, int64_t base, int nq,
                             float* D, int64_t* I, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)(nq < 4096 ? nq : 4096)), dim3(256), 0, st, rows, region, cnt, exact, lims, base, nq, D, I);
    return hipGetLastError();
}

template <bool L2>
__device__ __forceinline__ bool range_keep(double s, float radius, float& df) {
    df = (float)s;
    return L2 ? df < radius : df > radius;
}

// exact path, counting: one workgroup per listed query over its row of n scores
template <bool L2>
__global__ __launch_bounds__(256) void range_count_kernel(const int* qlist, int64_t n, const double* sc, float radius, int* cnt) {
    __shared__ int tot;
    const int f = blockIdx.x;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int c = 0;
    float df;
    for (int64_t j = threadIdx.x; j < n; j += 256) c += range_keep<L2>(sc[(int64_t)f * n + j], radius, df) ? 1 : 0;
    atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) cnt[qlist[f]] = tot;
}

// exact path, writing: an ordered compaction of the query's row (a ballot per wave, the four waves' counts through LDS)
template <bool L2>
__global__ __launch_bounds__(256) void range_emit_exact_kernel(const int* qlist, int64_t n, const double* sc, float radius, const int64_t* lims,
                                                               int64_t base, float* D, int64_t* I) {
    __shared__ int wsum[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t o = lims[qlist[f]] - base;
    for (int64_t j0 = 0; j0 < n; j0 += 256) {
        const int64_t j = j0 + tid;
        float df = 0.f;
        const bool keep = j < n && range_keep<L2>(sc[(int64_t)f * n + j], radius, df);
        const u64 b = __ballot(keep);
        const int pre = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { off += i < w ? wsum[i] : 0; tot += wsum[i]; }
        if (keep) { D[o + off + pre] = df; I[o + off + pre] = j; }
        __syncthreads();
        o += tot;
    }
}

hipError_t launch_range_count(int metric, const int* qlist, int m, int64_t n, const double* sc, float radius, int* cnt, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (metric) hipLaunchKernelGGL(range_count_kernel<true>, dim3(m), dim3(256), 0, st, qlist, n, sc, radius, cnt);
    else hipLaunchKernelGGL(range_count_kernel<false>, dim3(m), dim3(256), 0, st, qlist, n, sc, radius, cnt);
    return hipGetLastError();
}

hipError_t launch_range_emit_exact(int metric, const int* qlist, int m, int64_t n, const double* sc, float radius, const int64_t* lims,
                                   int64_t base, float* D, int64_t* I, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (metric) hipLaunchKernelGGL(range_emit_exact_kernel<true>, dim3(m), dim3(256), 0, st, qlist, n, sc, radius, lims, base, D, I);
    else hipLaunchKernelGGL(range_emit_exact_kernel<false>, dim3(m), dim3(256), 0, st, qlist, n, sc, radius, lims, base, D, I);
    return hipGetLastError();
}

}  // namespace trx
