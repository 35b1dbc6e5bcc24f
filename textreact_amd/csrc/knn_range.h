// knn_range.h -- the kernels of the range search (include/trx_knn.h: trx_index_range_search), knn_range.hip.  Internal.
//
// A range query is a fixed-threshold scan: every query's threshold is a key below which no row can satisfy the predicate
// (range_seed_kernel), the scan lists every row that reaches it, the listed rows are re-scored exactly and filtered
// (range_rescore_kernel), and the survivors go to a CSR result in ascending id (range_lims_kernel, range_emit_kernel).  A query
// whose lists overflowed takes the exact fp64 scan of the whole index (launch_exact_scores, then range_count_kernel and
// range_emit_exact_kernel).  DESIGN.md section 11.
#pragma once
#include "knn_common.h"

namespace trx {

constexpr int RANGE_MAX_SPLITS = 4;       // corpus splits of a range scan: at most 4 x 8 lists x 127 = 4,064 listed rows per query
constexpr int RANGE_LIST_MAX = RANGE_MAX_SPLITS * LISTS_PER_SPLIT * 127;
constexpr int RANGE_ROWS_MAX = 4096;      // a query's surviving rows, sorted by id in LDS; more of them: the exact path

struct RangeParams {
    const u64* cand;          // the scan's lists (ScanParams.cand / cand_cnt / cand_thr), nlists per query, by query number
    const u32* cand_cnt;
    const u64* cand_thr;
    u64* rows;                // [nq][nlists * cap_alloc]: a query's surviving rows, (id << 32 | float bits of D), ascending id --
                              // written over the query's own lists once they have been read
    int nlists;
    int cap_alloc;
    const void* corpus_orig;  // exact values: bf16 [..][ld_c] or f32 [..][ld_c]
    int64_t ld_c;
    const void* query_orig;   // exact query values, bf16 or f32, row stride ld_q
    int64_t ld_q;
    int corpus_is_bf16;
    int query_is_bf16;
    int d;
    int metric;
    int nq;
    int64_t n;                // corpus rows: ids >= n are pad rows of the last tile
    float radius;
    const float* qnorm2;      // fp32 |x_q|^2 (hostile queries: knn_common.h)
    const float* seed;        // [nq] the key every listed row reaches (range_seed_kernel)
    const int* special;       // the index's hostile rows (sorted ids): never listed here, scored against every query
    int nspecial;
    int* cnt;                 // [nq] out: results of the query (fast path; the exact path fills it later)
    int* exact;               // [nq] out: 1 = the query takes the exact path
    int* xlist;               // out: those queries ...
    int* nx;                  // ... and their number (zeroed by the caller)
};

// seed[q] and the scan's shared thresholds g_thr (all four slots) from the radius: the key of a row that satisfies the predicate
// exceeds |x|^2 - radius (L2) / radius (IP), lowered by twice the query's key error bound (knn_select.hip's eps_q) and an
// allowance for the fp32 rounding of D.  A hostile query gets +inf: it lists nothing and takes the exact path.
hipError_t launch_range_seeds(int metric, const void* q, int is_bf, int64_t nq, int d, double radius, const float* qnorm2, float eps_rel,
                              float eps_round, float ymax_norm2, const float* qerr2, float yerr2_max, float* seed, u32* g_thr, hipStream_t st);
hipError_t launch_range_rescore(const RangeParams& p, hipStream_t st);
// lims[i] = base + sum of cnt[0 .. i), i = 0 .. nq (one workgroup)
hipError_t launch_range_lims(const int* cnt, int nq, int64_t base, int64_t* lims, hipStream_t st);
// the fast path's rows into the CSR output D / I (positions lims[q] - base)
hipError_t launch_range_emit(const u64* rows, int region, const int* cnt, const int* exact, const int64_t* lims, int64_t base, int nq,
                             float* D, int64_t* I, hipStream_t st);
// the exact path: sc[f][n] canonical scores of the queries qlist[0 .. m) -> cnt[qlist[f]] ...
hipError_t launch_range_count(int metric, const int* qlist, int m, int64_t n, const double* sc, float radius, int* cnt, hipStream_t st);
// ... and, once lims is known, their rows in ascending id
hipError_t launch_range_emit_exact(int metric, const int* qlist, int m, int64_t n, const double* sc, float radius, const int64_t* lims,
                                   int64_t base, float* D, int64_t* I, hipStream_t st);
// the canonical scores alone (knn_select.hip): sc[f][n] for the queries of qlist (null: f itself)
hipError_t launch_exact_scores(int metric, int cbf, int qbf, const int* qlist, int nf, const int* nf_dev, int64_t n,
                               const void* corpus, int64_t ld_c, const void* queries, int64_t ld_q, int d, double* sc, hipStream_t st);

}  // namespace trx
