// rcp_summary.hip -- summaries of a profile matrix that stays in HBM: what every consumer of
// `$profile` in the reference computes from it again (R/plot.R):
//   calcPlotProfiles / calcDesignPlotProfiles   apply(profile, 2, mean) and sd      plot.R:949-1033
//   orderProfiles / orderProfilesByDesign       apply(profile, 1, sum|max|mean)      plot.R:1035-1330
// both after the optional log2(x + 1) (plot.R:953-956).  The matrix is the one rcp_plan_execute
// wrote: column c at mat + c * ld, rows 0 .. n_rows - 1 of it; rows n_rows .. ld - 1 are padding
// and are never loaded.
//
// Numerics contract (DESIGN.md "Device summaries"): no floating-point atomics anywhere; every
// reduction has a shape fixed by (n_rows, n_cols) alone, so results are bit-identical from run to
// run, on any stream, whatever else the device runs.  A standard deviation is always the sum of
// squared deviations about a mean (two passes over values held in registers, then Chan's pairwise
// merge of (n, mean, M2) partials) -- never sum(x^2) - n * mean^2.
//
// Column statistics (rcp_colstats_kernel): one workgroup of 256 lanes per (column, slab of 4096
// rows).  A lane loads 8 pairs of adjacent rows, 16 bytes each (pair p of the slab belongs to lane
// p % 256, so a wave's load is 1 KiB of one column), keeps the 16 values in registers, and the
// workgroup reduces, per group present in the slab: sum and count -> the slab's mean -> the sum of
// squared deviations about it.  Wave sums are xor butterflies, the 4 waves' results are added in
// wave order.  The slab's (n, mean, M2) goes to a partial slab; rcp_colstats_final_kernel merges
// the slabs of a (group, column) in slab order.  The matrix is read exactly once.
//
// Row statistics (rcp_rowstats_kernel): one workgroup per 64 rows; lane l of every wave owns row
// l of the tile, so each column step of a wave is one coalesced 512-byte line; the 4 waves take
// 4 contiguous quarters of the columns, in chunks of 8 independent loads, and their partials are
// merged in wave order.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/recoup_amd.h"
#include "rcp_summary.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPairs = kSumColSlabRows / (2 * kBlock);  // 16-byte loads per lane
static_assert(kPairs * 2 * kBlock == kSumColSlabRows, "slab = lanes x pairs x 2");
constexpr int kRowChunk = 8;  // columns a lane of the row kernel loads before it reduces them

__device__ __forceinline__ double wave_sum(double v) {
    // xor butterfly: IEEE addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over the workgroup, the same bits in every lane.  sh is [2][kWaves]; successive calls
// alternate the half they use (phase), which makes one barrier per call enough: a wave can only
// reach the write of call i + 2 after every wave has passed the barrier of call i + 1, i.e. after
// every wave has read call i's half.
__device__ __forceinline__ double block_sum(double v, double (*sh)[kWaves], int& phase) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[phase][threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[phase][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r += sh[phase][w];
    phase ^= 1;
    return r;
}

// two sums at once (one barrier), in the same alternation
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*sa)[kWaves], double (*sb)[kWaves],
                                           int& phase) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        sa[phase][threadIdx.x >> 6] = a;
        sb[phase][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = sa[phase][0];
    b = sb[phase][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        a += sa[phase][w];
        b += sb[phase][w];
    }
    phase ^= 1;
}

template <bool LOG>
__device__ __forceinline__ double tr(double v) {
    return LOG ? log2(v + 1.0) : v;  // plot.R:953-956: x + 1, then log2
}

template <bool GROUPED, bool LOG>
__global__ void __launch_bounds__(kBlock)
rcp_colstats_kernel(const double* __restrict__ mat, int64_t n_rows, int64_t n_cols, int64_t ld,
                    const int32_t* __restrict__ gid, int32_t n_groups, double* __restrict__ pn,
                    double* __restrict__ pmean, double* __restrict__ pm2, unsigned long long* __restrict__ mask_out) {
    __shared__ double sh_a[2][kWaves];
    __shared__ double sh_b[2][kWaves];
    __shared__ unsigned long long sh_mask;
    const int t = threadIdx.x;
    const int64_t slab = (int64_t)blockIdx.x / n_cols;
    const int64_t c = (int64_t)blockIdx.x - slab * n_cols;
    const int64_t lo = slab * kSumColSlabRows;
    const int64_t hi = min(lo + (int64_t)kSumColSlabRows, n_rows);
    const double* col = mat + c * ld;
    // lo is even, so every pair of the slab is 16-byte aligned exactly when col + lo is (a padded
    // ld on an aligned base: always); otherwise the same pairs are loaded as two 8-byte halves
    const bool aligned = (reinterpret_cast<uintptr_t>(col + lo) & 15) == 0;
    if (GROUPED && t == 0) sh_mask = 0ull;

    double x[2 * kPairs];
    int g[2 * kPairs];  // group of the value; -1: not a row of the matrix, or a row no group holds
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
        } else if (r < hi) {
            a = col[r];
        }
        x[2 * k] = tr<LOG>(a);
        x[2 * k + 1] = tr<LOG>(b);
        int ga = r < hi ? 0 : -1, gb = r + 1 < hi ? 0 : -1;
        if (GROUPED) {
            if (ga == 0) {
                ga = gid[r];
                if (ga < 0 || ga >= n_groups) ga = -1;
            }
            if (gb == 0) {
                gb = gid[r + 1];
                if (gb < 0 || gb >= n_groups) gb = -1;
            }
        }
        g[2 * k] = ga;
        g[2 * k + 1] = gb;
    }

    int phase = 0;
    if (!GROUPED) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * kPairs; ++j) s += g[j] == 0 ? x[j] : 0.0;
        const double n = (double)(hi - lo);
        const double mean = block_sum(s, sh_a, phase) / n;
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * kPairs; ++j) {
            const double d = g[j] == 0 ? x[j] - mean : 0.0;
            q += d * d;
        }
        q = block_sum(q, sh_a, phase);
        if (t == 0) {
            const int64_t i = slab * n_cols + c;
            pn[i] = n;
            pmean[i] = mean;
            pm2[i] = q;
        }
        return;
    }

    // groups present in the slab (integer atomics on LDS: the result does not depend on order)
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < 2 * kPairs; ++j)
        if (g[j] >= 0) mine |= 1ull << g[j];
    __syncthreads();  // sh_mask = 0 is visible
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mine |= __shfl_xor(mine, off, 64);
    if ((t & 63) == 0 && mine) atomicOr(&sh_mask, mine);
    __syncthreads();
    const unsigned long long present = sh_mask;
    if (t == 0 && c == 0) mask_out[slab] = present;
    for (unsigned long long m = present; m; m &= m - 1) {
        const int gg = __ffsll((long long)m) - 1;
        double s = 0.0, cnt = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * kPairs; ++j) {
            s += g[j] == gg ? x[j] : 0.0;
            cnt += g[j] == gg ? 1.0 : 0.0;
        }
        block_sum2(s, cnt, sh_a, sh_b, phase);
        const double n = cnt;
        const double mean = s / n;
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 2 * kPairs; ++j) {
            const double d = g[j] == gg ? x[j] - mean : 0.0;
            q += d * d;
        }
        q = block_sum(q, sh_a, phase);
        if (t == 0) {
            const int64_t i = (slab * n_groups + gg) * n_cols + c;
            pn[i] = n;
            pmean[i] = mean;
            pm2[i] = q;
        }
    }
}

// Chan, Golub & LeVeque's merge of (n, mean, M2) with (nb, mb, qb)
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& q, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (n == 0.0) {
        n = nb;
        mean = mb;
        q = qb;
        return;
    }
    const double nn = n + nb;
    const double d = mb - mean;
    mean += d * (nb / nn);
    q += qb + d * d * (n * nb / nn);
    n = nn;
}

__global__ void __launch_bounds__(kBlock)
rcp_colstats_final_kernel(int64_t n_slabs, int64_t n_cols, int32_t n_groups, const double* __restrict__ pn,
                          const double* __restrict__ pmean, const double* __restrict__ pm2,
                          const unsigned long long* __restrict__ mask, double* __restrict__ mean_out,
                          double* __restrict__ sd_out, int64_t* __restrict__ count_out) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int gg = blockIdx.y;
    if (c >= n_cols) return;
    double n = 0.0, mean = 0.0, q = 0.0;
    for (int64_t b = 0; b < n_slabs; ++b) {
        if (mask && !((mask[b] >> gg) & 1ull)) continue;
        const int64_t i = (b * n_groups + gg) * n_cols + c;
        chan_merge(n, mean, q, pn[i], pmean[i], pm2[i]);
    }
    const int64_t o = (int64_t)gg * n_cols + c;
    // R: mean(numeric(0)) is NaN, sd of fewer than two values is NA
    if (mean_out) mean_out[o] = n > 0.0 ? mean : (double)NAN;
    if (sd_out) sd_out[o] = n > 1.0 ? sqrt(q / (n - 1.0)) : (double)NAN;
    if (count_out) count_out[o] = (int64_t)n;
}

template <bool LOG, bool SD>
__global__ void __launch_bounds__(kBlock)
rcp_rowstats_kernel(const double* __restrict__ mat, int64_t n_rows, int64_t n_cols, int64_t ld,
                    double* __restrict__ o_sum, double* __restrict__ o_max, double* __restrict__ o_mean,
                    double* __restrict__ o_sd) {
    __shared__ double sh[5][kWaves][kSumRowTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kSumRowTile + lane;
    const bool active = row < n_rows;
    const int64_t per = (n_cols + kWaves - 1) / kWaves;
    const int64_t c0 = min((int64_t)w * per, n_cols), c1 = min(c0 + per, n_cols);
    const double* p = mat + row;
    double sum = 0.0, mx = -INFINITY, n = 0.0, mean = 0.0, q = 0.0;
    for (int64_t c = c0; c < c1; c += kRowChunk) {
        const int nb = (int)min((int64_t)kRowChunk, c1 - c);
        double x[kRowChunk];
#pragma unroll
        for (int j = 0; j < kRowChunk; ++j) x[j] = (active && j < nb) ? tr<LOG>(p[(c + j) * ld]) : 0.0;
        double cs = 0.0;
#pragma unroll
        for (int j = 0; j < kRowChunk; ++j) {
            cs += x[j];
            if (j < nb) mx = fmax(mx, x[j]);
        }
        sum += cs;
        if (SD) {
            const double cm = cs / (double)nb;
            double cq = 0.0;
#pragma unroll
            for (int j = 0; j < kRowChunk; ++j) {
                const double d = j < nb ? x[j] - cm : 0.0;
                cq += d * d;
            }
            chan_merge(n, mean, q, (double)nb, cm, cq);
        }
    }
    sh[0][w][lane] = sum;
    sh[1][w][lane] = mx;
    if (SD) {
        sh[2][w][lane] = n;
        sh[3][w][lane] = mean;
        sh[4][w][lane] = q;
    }
    __syncthreads();
    if (w != 0 || !active) return;
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
        sum += sh[0][k][lane];
        mx = fmax(mx, sh[1][k][lane]);
        if (SD) chan_merge(n, mean, q, sh[2][k][lane], sh[3][k][lane], sh[4][k][lane]);
    }
    if (o_sum) o_sum[row] = sum;
    if (o_max) o_max[row] = mx;
    if (o_mean) o_mean[row] = sum / (double)n_cols;
    if (SD && o_sd) o_sd[row] = n > 1.0 ? sqrt(q / (n - 1.0)) : (double)NAN;
}

__global__ void __launch_bounds__(kBlock)
rcp_order_keys_kernel(const double* __restrict__ stat, int32_t n_samples, int64_t n_rows, int what, int decreasing,
                      const int32_t* __restrict__ gid, int32_t n_groups, double* __restrict__ d_key,
                      uint64_t* __restrict__ skey, int32_t* __restrict__ idx) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    // over all samples: the sum of sums, the max of maxes (byMax draws sample(mp, 1) among equal
    // maxima, plot.R:1126-1133, and returns the same value whichever it draws: no RNG here), the
    // mean of means (plot.R:1082-1085, :1125-1135, :1170-1173), samples in list order
    double v = stat[r];
    for (int32_t s = 1; s < n_samples; ++s) {
        const double y = stat[(int64_t)s * n_rows + r];
        v = what == RCP_KEY_MAX ? fmax(v, y) : v + y;
    }
    if (what == RCP_KEY_AVG && n_samples > 1) v = v / (double)n_samples;
    if (d_key) d_key[r] = v;
    bool held = true;
    if (gid) {
        const int32_t gg = gid[r];
        held = gg >= 0 && gg < n_groups;
    }
    // R compares -0.0 and 0.0 equal: one sortable form for both.  Descending is the ascending
    // order of the complemented form, so ties keep row order in both directions.
    const uint64_t k = rcp_sort_key(v == 0.0 ? 0.0 : v);
    skey[r] = held ? (decreasing ? ~k : k) : 0ull;  // rows no group holds stay in row order
    idx[r] = (int32_t)r;
}

__global__ void __launch_bounds__(kBlock)
rcp_order_groups_kernel(int64_t n_rows, const int32_t* __restrict__ idx, const int32_t* __restrict__ gid,
                        int32_t n_groups, uint64_t* __restrict__ gkey) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t gg = gid[idx[i]];
    gkey[i] = (gg >= 0 && gg < n_groups) ? (uint64_t)gg : (uint64_t)n_groups;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" hipError_t rcp_launch_colstats(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                                          const int32_t* d_group, int32_t n_groups, double* pn, double* pmean,
                                          double* pm2, unsigned long long* mask, hipStream_t stream) {
    const int64_t n_slabs = (n_rows + kSumColSlabRows - 1) / kSumColSlabRows;
    if (n_slabs == 0 || n_cols == 0) return hipSuccess;
    if (n_slabs * n_cols > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(n_slabs * n_cols)), block(kBlock);
#define RCP_COLSTATS(G, L)                                                                                       \
    hipLaunchKernelGGL((rcp_colstats_kernel<G, L>), grid, block, 0, stream, mat, n_rows, n_cols, ld, d_group, \
                       n_groups, pn, pmean, pm2, mask)
    if (d_group) {
        if (log2p1) RCP_COLSTATS(true, true); else RCP_COLSTATS(true, false);
    } else {
        if (log2p1) RCP_COLSTATS(false, true); else RCP_COLSTATS(false, false);
    }
#undef RCP_COLSTATS
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_colstats_final(int64_t n_slabs, int64_t n_cols, int32_t n_groups, const double* pn,
                                                const double* pmean, const double* pm2,
                                                const unsigned long long* mask, double* mean, double* sd,
                                                int64_t* count, hipStream_t stream) {
    if (n_cols == 0 || n_groups == 0) return hipSuccess;
    const dim3 grid(blocks_of(n_cols), (unsigned)n_groups), block(kBlock);
    hipLaunchKernelGGL(rcp_colstats_final_kernel, grid, block, 0, stream, n_slabs, n_cols, n_groups, pn, pmean, pm2,
                       mask, mean, sd, count);
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_rowstats(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                                          double* o_sum, double* o_max, double* o_mean, double* o_sd,
                                          hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const dim3 grid((unsigned)((n_rows + kSumRowTile - 1) / kSumRowTile)), block(kBlock);
#define RCP_ROWSTATS(L, S) \
    hipLaunchKernelGGL((rcp_rowstats_kernel<L, S>), grid, block, 0, stream, mat, n_rows, n_cols, ld, o_sum, o_max, o_mean, o_sd)
    if (o_sd) {
        if (log2p1) RCP_ROWSTATS(true, true); else RCP_ROWSTATS(false, true);
    } else {
        if (log2p1) RCP_ROWSTATS(true, false); else RCP_ROWSTATS(false, false);
    }
#undef RCP_ROWSTATS
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_order_keys(const double* stat, int32_t n_samples, int64_t n_rows, int what,
                                            int decreasing, const int32_t* d_group, int32_t n_groups, double* d_key,
                                            uint64_t* skey, int32_t* idx, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rcp_order_keys_kernel, dim3(blocks_of(n_rows)), dim3(kBlock), 0, stream, stat, n_samples,
                       n_rows, what, decreasing, d_group, n_groups, d_key, skey, idx);
    return hipGetLastError();
}

extern "C" hipError_t rcp_launch_order_groups(int64_t n_rows, const int32_t* idx, const int32_t* d_group,
                                              int32_t n_groups, uint64_t* gkey, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rcp_order_groups_kernel, dim3(blocks_of(n_rows)), dim3(kBlock), 0, stream, n_rows, idx,
                       d_group, n_groups, gkey);
    return hipGetLastError();
}
