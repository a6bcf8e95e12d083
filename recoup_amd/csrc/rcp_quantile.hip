// rcp_quantile.hip -- exact order statistics of a profile matrix that stays in HBM: what the
// reference computes with quantile(profile, q) for the heatmap colour limits (R/plot.R:510-545) and
// with apply(profile, 2, median) / apply(profile, 2, mad) for median curves (R/plot.R:976-988),
// after the optional log2(x + 1).  Semantics: include/recoup_amd.h (R's quantile.default type 7,
// median.default and mad restated from R's source as remembered; R is not available here).
//
// Numerics contract (DESIGN.md "Device summaries"): no floating-point atomics anywhere; every
// reduction has a shape fixed by (n_rows, n_cols) alone, so results are bit-identical from run to
// run, on any stream, whatever else the device runs.  Here the only atomics are integer adds, ors
// and mins, whose results do not depend on arrival order, and selection is exact.
//
// Key: rcp_sort_key (sign flip) of the element, with -0.0 folded onto 0.0 and every NaN of either
// sign mapped to the one key above +Inf (all ones).  A segment is a column, or the whole matrix
// (segment 0).  A call selects x_(lo) of up to kQMaxProbs probabilities per segment at once, one
// "slot" each, by a most-significant-digit radix selection in kQPasses passes of kQBits bits:
//
//   rcp_qhist_kernel   streams the matrix once with the column-statistics kernel's load shape: a
//                      workgroup of 256 lanes takes (column, slab of kSumColSlabRows rows) units,
//                      a lane 8 pairs of adjacent rows per unit, 16 bytes each when aligned and the
//                      same pairs as 8-byte halves when not.  It counts the pass's digit of every
//                      key that matches its slot's prefix into a histogram in LDS (kQBins counters
//                      per slot: 8 KiB for 8 slots) and flushes the non-zero counters with integer
//                      atomics into the segment's global histogram.  A workgroup takes
//                      kQUnitsPerGroup consecutive slabs of one column, or in whole-matrix scope as
//                      many units as leave about kQMatrixGroups workgroups: every workgroup of that
//                      scope flushes into the same counters, and one flush per 4096 elements would
//                      put a hundred million atomics on 2048 addresses.
//                      Slots whose prefixes are equal share one histogram (RcpQState::rep): on pass 0
//                      all of them, and the ladder 0.95 .. 0.999 for several passes more.
//                      Ties are the common case (coverage is mostly zeros, and the first digit --
//                      sign and high exponent bits -- is shared by nearly all of any data): before a
//                      lane adds to LDS the wave peels off, kQPeel times, the digit of its first
//                      remaining lane with one add of the ballot's population count; the lanes left
//                      add singly.  After the first passes few keys match any prefix: a slot ands
//                      its 16 match bits per lane first, and one ballot skips the unit for it.
//   rcp_qpick_kernel   one workgroup per segment, one wave per slot: a wave scan over the slot's
//                      histogram finds the digit that holds the rank, extends the prefix, lowers the
//                      rank by the count below, zeroes the histogram and regroups equal prefixes.
//                      After the last pass it knows less = #{x < x_(lo)} and ceq = #{x == x_(lo)},
//                      so x_(hi) = x_(lo) when hi <= less + ceq; otherwise x_(hi) is the smallest
//                      key above x_(lo):
//   rcp_qsucc_kernel   one more streaming pass taking an integer min of the keys above x_(lo)
//                      (skipped when no requested probability interpolates).
//   rcp_qfinal_kernel  turns keys back into doubles and interpolates with separately rounded
//                      products and sum (contraction switched off for that kernel: never an FMA).
//
// Selection ends correctly when every remaining candidate is equal: the passes simply follow the
// one occupied digit.  Scratch is the histograms and per-(segment, slot) state, never a copy of
// the matrix.  Counters are 32-bit: the host refuses segments of 2^32 or more elements.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/recoup_amd.h"
#include "rcp_summary.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPairs = kSumColSlabRows / (2 * kBlock);  // 16-byte loads per lane and unit
static_assert(kPairs * 2 * kBlock == kSumColSlabRows, "slab = lanes x pairs x 2");
static_assert(kQBins == kBlock, "lane t zeroes and flushes counter t of every slot");
static_assert(kQBins == 4 * 64, "a wave of the pick kernel holds 4 counters per lane");
constexpr int kQPeel = 3;  // shared digits a wave adds with one atomic each before lanes add singly
constexpr unsigned long long kNanKey = ~0ull;

template <bool LOG, bool DEV>
__device__ __forceinline__ unsigned long long qkey(double v, double center) {
    double y = LOG ? log2(v + 1.0) : v;  // plot.R:481-486, :953-956: x + 1, then log2
    if (DEV) y = fabs(y - center);
    if (y != y) return kNanKey;
    return rcp_sort_key(y == 0.0 ? 0.0 : y);
}

__device__ __forceinline__ double qvalue(unsigned long long k) {  // inverse of rcp_sort_key
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// The units [u0, u1) of workgroup w (unit u = column u / n_slabs, slab u % n_slabs) and its segment
__device__ __forceinline__ void group_units(int64_t w, int32_t scope, int64_t n_slabs, int64_t n_units,
                                            int64_t upg, int64_t gpc, int64_t& u0, int64_t& u1, int64_t& seg) {
    if (scope == RCP_QUANTILE_COLS) {
        const int64_t c = w / gpc;
        u0 = c * n_slabs + (w - c * gpc) * upg;
        u1 = min(u0 + upg, (c + 1) * n_slabs);
        seg = c;
    } else {
        u0 = w * upg;
        u1 = min(u0 + upg, n_units);
        seg = 0;
    }
}

// Keys of the 16 elements of lane t in unit u; bit i of the result: key[i] is a row of the matrix
template <bool LOG, bool DEV>
__device__ __forceinline__ unsigned load_keys(const double* __restrict__ mat, int64_t n_rows, int64_t ld,
                                              int64_t n_slabs, int64_t u, double center,
                                              unsigned long long (&key)[2 * kPairs]) {
    const int t = threadIdx.x;
    const int64_t c = u / n_slabs;
    const int64_t lo = (u - c * n_slabs) * kSumColSlabRows;
    const int64_t hi = min(lo + (int64_t)kSumColSlabRows, n_rows);
    const double* col = mat + c * ld;
    // lo is even: every pair of the slab is 16-byte aligned exactly when col + lo is
    const bool aligned = (reinterpret_cast<uintptr_t>(col + lo) & 15) == 0;
    double x[2 * kPairs];
    unsigned valid = 0;
#pragma unroll
    for (int k = 0; k < kPairs; ++k) {
        const int64_t r = lo + 2 * (int64_t)(t + kBlock * k);
        double a = 0.0, b = 0.0;
        if (r + 1 < hi) {
            if (aligned) {
                const double2 v = *reinterpret_cast<const double2*>(col + r);
                a = v.x;
                b = v.y;
            } else {
                a = col[r];
                b = col[r + 1];
            }
            valid |= 3u << (2 * k);
        } else if (r < hi) {
            a = col[r];
            valid |= 1u << (2 * k);
        }
        x[2 * k] = a;
        x[2 * k + 1] = b;
    }
#pragma unroll
    for (int i = 0; i < 2 * kPairs; ++i) key[i] = qkey<LOG, DEV>(x[i], center);
    return valid;
}

// One count for every lane with m set, into h[digit]: shared digits first, one atomic per digit
__device__ __forceinline__ void wave_count(uint32_t* h, bool m, uint32_t digit) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(m);
#pragma unroll
    for (int round = 0; round < kQPeel; ++round) {
        if (rem == 0ull) return;  // (wave-uniform)
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t d = (uint32_t)__shfl((int)digit, leader, 64);
        const unsigned long long same = __ballot(m && digit == d);
        if (lane == leader) atomicAdd(&h[d], (uint32_t)__popcll(same));
        rem &= ~same;
        m = m && digit != d;
    }
    if (m) atomicAdd(&h[digit], 1u);
}

template <bool LOG, bool DEV>
__global__ void __launch_bounds__(kBlock)
rcp_qhist_kernel(const double* __restrict__ mat, int64_t n_rows, int64_t ld, int64_t n_slabs, int64_t n_units,
                 int64_t upg, int64_t gpc, const double* __restrict__ center, int32_t scope, int32_t np, int32_t pass,
                 const RcpQState* __restrict__ state, uint32_t* __restrict__ hist, uint32_t* __restrict__ nanflag) {
    __shared__ uint32_t sh_hist[kQMaxProbs * kQBins];
    __shared__ unsigned long long sh_prefix[kQMaxProbs];
    const int t = threadIdx.x;
    int64_t u0, u1, seg;
    group_units(blockIdx.x, scope, n_slabs, n_units, upg, gpc, u0, u1, seg);
    // slots that count for themselves (on pass 0 all share slot 0's histogram: nothing is chosen yet)
    unsigned active = 0;
    for (int j = 0; j < np; ++j) {
        if (pass == 0) {
            active |= j == 0 ? 1u : 0u;
        } else {
            const RcpQState s = state[seg * np + j];
            if (s.rep == j) active |= 1u << j;
            if (t == 0) sh_prefix[j] = s.prefix;
        }
    }
    for (int j = 0; j < np; ++j)
        if ((active >> j) & 1u) sh_hist[j * kQBins + t] = 0u;
    __syncthreads();
    const double ctr = DEV ? center[seg] : 0.0;
    const int shift = 64 - kQBits * (pass + 1);
    bool saw_nan = false;
    for (int64_t u = u0; u < u1; ++u) {
        unsigned long long key[2 * kPairs];
        const unsigned valid = load_keys<LOG, DEV>(mat, n_rows, ld, n_slabs, u, ctr, key);
        if (pass == 0) {
#pragma unroll
            for (int i = 0; i < 2 * kPairs; ++i) saw_nan |= ((valid >> i) & 1u) && key[i] == kNanKey;
        }
        for (int j = 0; j < np; ++j) {
            if (!((active >> j) & 1u)) continue;
            const unsigned long long pf = pass == 0 ? 0ull : sh_prefix[j];
            // bit i: element i is a row of the matrix and the digits above this pass's equal the
            // prefix's (on pass 0 there are none).  After the first passes few keys match any prefix:
            // one ballot per slot then skips the unit, instead of one per element.
            unsigned mm = valid;
            if (pass != 0) {
#pragma unroll
                for (int i = 0; i < 2 * kPairs; ++i)
                    if (((key[i] ^ pf) >> (shift + kQBits)) != 0ull) mm &= ~(1u << i);
            }
            if (__ballot(mm != 0u) == 0ull) continue;  // (wave-uniform)
#pragma unroll
            for (int i = 0; i < 2 * kPairs; ++i) {
                wave_count(sh_hist + j * kQBins, (mm >> i) & 1u, (uint32_t)(key[i] >> shift) & (kQBins - 1));
                // one element's ballots at a time: interleaved, the 16 elements' lane masks do not
                // fit the scalar registers
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __syncthreads();
    for (int j = 0; j < np; ++j) {
        if (!((active >> j) & 1u)) continue;
        const uint32_t v = sh_hist[j * kQBins + t];
        if (v) atomicAdd(&hist[(seg * np + j) * kQBins + t], v);
    }
    if (pass == 0 && __ballot(saw_nan) != 0ull && (t & 63) == 0) atomicOr(&nanflag[seg], 1u);
}

__global__ void __launch_bounds__(64 * kQMaxProbs)
rcp_qpick_kernel(int32_t np, int32_t pass, RcpQRanks ranks, RcpQState* __restrict__ state,
                 uint32_t* __restrict__ hist) {
    __shared__ unsigned long long sh_prefix[kQMaxProbs];
    __shared__ int sh_need[kQMaxProbs];
    const int64_t seg = blockIdx.x;
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;  // blockDim.x = 64 * np: wave j is slot j
    RcpQState s;
    if (pass == 0) {
        s.prefix = 0ull;
        s.less = 0ull;
        s.k = ranks.k[j];
        s.ceq = 0u;
        s.rep = 0;
        s.pad = 0;
    } else {
        s = state[seg * np + j];
    }
    const uint4 c = reinterpret_cast<const uint4*>(hist + (seg * np + s.rep) * kQBins)[lane];
    const uint32_t sum = c.x + c.y + c.z + c.w;
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += v;
    }
    const uint32_t excl = incl - sum;
    __syncthreads();  // every slot has read the histogram it shares
    if (s.rep == j) reinterpret_cast<uint4*>(hist + (seg * np + j) * kQBins)[lane] = make_uint4(0u, 0u, 0u, 0u);
    const bool mine = s.k >= excl && s.k < incl;  // exactly one lane: the rank is below the slot's total
    const bool last = pass == kQPasses - 1;
    if (mine) {
        uint32_t kk = s.k - excl, d = 0u, cnt = c.x;
        if (kk >= cnt) {
            kk -= cnt;
            d = 1u;
            cnt = c.y;
            if (kk >= cnt) {
                kk -= cnt;
                d = 2u;
                cnt = c.z;
                if (kk >= cnt) {
                    kk -= cnt;
                    d = 3u;
                    cnt = c.w;
                }
            }
        }
        s.less += (unsigned long long)(s.k - kk);
        s.k = kk;
        s.ceq = cnt;
        s.prefix |= (unsigned long long)(4u * (uint32_t)lane + d) << (64 - kQBits * (pass + 1));
        sh_prefix[j] = s.prefix;
        // after the last pass: hi = lo + 1 = ranks.k + 2 lies beyond the tie of x_(lo)
        sh_need[j] = last && ranks.interp[j] && (unsigned long long)ranks.k[j] + 2ull > s.less + s.ceq;
    }
    __syncthreads();
    if (mine) {
        int rep = j;
        for (int i = j - 1; i >= 0; --i)
            if (sh_prefix[i] == s.prefix && (!last || sh_need[i])) rep = i;
        s.rep = (last && !sh_need[j]) ? -1 : rep;
        state[seg * np + j] = s;
    }
}

template <bool LOG, bool DEV>
__global__ void __launch_bounds__(kBlock)
rcp_qsucc_kernel(const double* __restrict__ mat, int64_t n_rows, int64_t ld, int64_t n_slabs, int64_t n_units,
                 int64_t upg, int64_t gpc, const double* __restrict__ center, int32_t scope, int32_t np,
                 const RcpQState* __restrict__ state, unsigned long long* __restrict__ succ) {
    __shared__ unsigned long long sh_prefix[kQMaxProbs];
    __shared__ unsigned long long sh_min[kQMaxProbs][kWaves];
    const int t = threadIdx.x;
    int64_t u0, u1, seg;
    group_units(blockIdx.x, scope, n_slabs, n_units, upg, gpc, u0, u1, seg);
    unsigned active = 0;
    for (int j = 0; j < np; ++j) {
        const RcpQState s = state[seg * np + j];
        if (s.rep == j) active |= 1u << j;
        if (t == 0) sh_prefix[j] = s.prefix;
    }
    if (active == 0u) return;  // (uniform over the workgroup)
    __syncthreads();
    const double ctr = DEV ? center[seg] : 0.0;
    unsigned long long best[kQMaxProbs];
#pragma unroll
    for (int j = 0; j < kQMaxProbs; ++j) best[j] = kNanKey;
    for (int64_t u = u0; u < u1; ++u) {
        unsigned long long key[2 * kPairs];
        const unsigned valid = load_keys<LOG, DEV>(mat, n_rows, ld, n_slabs, u, ctr, key);
#pragma unroll
        for (int j = 0; j < kQMaxProbs; ++j) {
            if (!((active >> j) & 1u)) continue;
            const unsigned long long pf = sh_prefix[j];
#pragma unroll
            for (int i = 0; i < 2 * kPairs; ++i)
                if (((valid >> i) & 1u) && key[i] > pf) best[j] = min(best[j], key[i]);
        }
    }
#pragma unroll
    for (int j = 0; j < kQMaxProbs; ++j) {
        if (!((active >> j) & 1u)) continue;
        unsigned long long b = best[j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) b = min(b, (unsigned long long)__shfl_xor((long long)b, off, 64));
        if ((t & 63) == 0) sh_min[j][t >> 6] = b;
    }
    __syncthreads();
    if (t < np && ((active >> t) & 1u)) {
        unsigned long long b = sh_min[t][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) b = min(b, sh_min[t][w]);
        if (b != kNanKey) atomicMin(&succ[seg * np + t], b);
    }
}

__global__ void __launch_bounds__(kBlock)
rcp_qfinal_kernel(int64_t n_out, int32_t np, RcpQRanks ranks, const RcpQState* __restrict__ state,
                  const unsigned long long* __restrict__ succ, const uint32_t* __restrict__ nanflag, int mad_scale,
                  double* __restrict__ q) {
    // Both products and the sum round separately (R on x86-64 does not fuse).  Plain operators under
    // this pragma: HIP's __dmul_rn / __dadd_rn are inline functions built with the default
    // contraction, and the compiler fuses them after inlining.
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_out) return;
    const int64_t seg = i / np;
    const int j = (int)(i - seg * np);
    const RcpQState s = state[i];
    const double lo = qvalue(s.prefix);
    double v = lo;
    if (s.rep >= 0) {  // x_(hi) lies above the tie of x_(lo): the smallest key above it
        const double hi = qvalue(succ[seg * np + s.rep]);
        const double h = ranks.h[j];
        if (hi != lo) v = (1.0 - h) * lo + h * hi;
    }
    if (mad_scale) v = 1.4826 * v;
    if (nanflag[seg]) v = (double)NAN;
    q[i] = v;
}

__global__ void __launch_bounds__(kBlock) rcp_qfill_nan_kernel(double* __restrict__ q, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) q[i] = (double)NAN;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

RcpQGeom rcp_quantile_geometry(int64_t n_rows, int64_t n_cols, int32_t scope) {
    RcpQGeom g;
    g.n_slabs = (n_rows + kSumColSlabRows - 1) / kSumColSlabRows;
    g.n_units = g.n_slabs * n_cols;
    g.units_per_group = kQUnitsPerGroup;
    if (scope == RCP_QUANTILE_COLS) {
        g.groups_per_col = (g.n_slabs + g.units_per_group - 1) / g.units_per_group;
        g.grid = g.groups_per_col * n_cols;
    } else {
        const int64_t spread = (g.n_units + kQMatrixGroups - 1) / kQMatrixGroups;
        if (spread > g.units_per_group) g.units_per_group = spread;
        g.groups_per_col = 0;
        g.grid = (g.n_units + g.units_per_group - 1) / g.units_per_group;
    }
    return g;
}

#define RCP_QSTREAM(KERNEL, ...)                                                                      \
    do {                                                                                              \
        if (center) {                                                                                 \
            if (log2p1) hipLaunchKernelGGL((KERNEL<true, true>), grid, block, 0, stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<false, true>), grid, block, 0, stream, __VA_ARGS__);      \
        } else {                                                                                      \
            if (log2p1) hipLaunchKernelGGL((KERNEL<true, false>), grid, block, 0, stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<false, false>), grid, block, 0, stream, __VA_ARGS__);     \
        }                                                                                             \
    } while (0)

extern "C" hipError_t rcp_launch_qhist(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                                       const double* center, int32_t scope, int32_t n_probs, int32_t pass,
                                       const RcpQState* state, uint32_t* hist, uint32_t* nanflag,
                                       hipStream_t stream) {
    const RcpQGeom g = rcp_quantile_geometry(n_rows, n_cols, scope);
    if (g.grid == 0) return hipSuccess;
    if (g.grid > 0x7fffffffLL || n_probs < 1 || n_probs > kQMaxProbs || pass < 0 || pass >= kQPasses)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)g.grid), block(kBlock);
    RCP_QSTREAM(rcp_qhist_kernel, mat, n_rows, ld, g.n_slabs, g.n_units, g.units_per_group, g.groups_per_col, center,
                scope, n_probs, pass, state, hist, nanflag);
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_qsucc(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                                       const double* center, int32_t scope, int32_t n_probs, const RcpQState* state,
                                       unsigned long long* succ, hipStream_t stream) {
    const RcpQGeom g = rcp_quantile_geometry(n_rows, n_cols, scope);
    if (g.grid == 0) return hipSuccess;
    if (g.grid > 0x7fffffffLL || n_probs < 1 || n_probs > kQMaxProbs) return hipErrorInvalidValue;
    const dim3 grid((unsigned)g.grid), block(kBlock);
    RCP_QSTREAM(rcp_qsucc_kernel, mat, n_rows, ld, g.n_slabs, g.n_units, g.units_per_group, g.groups_per_col, center,
                scope, n_probs, state, succ);
    return hipGetLastError();
}
#undef RCP_QSTREAM

extern "C" hipError_t rcp_launch_qpick(int64_t n_segments, int32_t n_probs, int32_t pass, const RcpQRanks* ranks,
                                       RcpQState* state, uint32_t* hist, hipStream_t stream) {
    if (n_segments == 0) return hipSuccess;
    if (n_segments > 0x7fffffffLL || n_probs < 1 || n_probs > kQMaxProbs || pass < 0 || pass >= kQPasses)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rcp_qpick_kernel, dim3((unsigned)n_segments), dim3(64 * n_probs), 0, stream, n_probs, pass,
                       *ranks, state, hist);
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_qfinal(int64_t n_segments, int32_t n_probs, const RcpQRanks* ranks,
                                        const RcpQState* state, const unsigned long long* succ,
                                        const uint32_t* nanflag, int mad_scale, double* q, hipStream_t stream) {
    const int64_t n = n_segments * n_probs;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcp_qfinal_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, stream, n, n_probs, *ranks, state, succ,
                       nanflag, mad_scale, q);
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_qfill_nan(double* q, int64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcp_qfill_nan_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, stream, q, n);
    return hipGetLastError();
}
