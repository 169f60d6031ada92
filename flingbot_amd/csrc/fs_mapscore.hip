// fs_mapscore.hip -- the rank statistics of recorded reward maps under the current weights, for a whole batch of images in ONE
// launch (flingbot_amd/trainops.py map_score; include/flingsim.h has the rule in full): what probe.map_stats computes on the host,
// map by map, from the dense value maps the eval forward wrote and the (pixel, label) lists of replay.MapSet.
//
//   fs_k_map_score   one workgroup of 256 threads per image.  The image's (p, y) -- p gathered from the dense map at the listed
//                    pixels -- go into LDS as float2 (32 KiB at 4096 labels), a position that is not counted (p or y not finite)
//                    as (NaN, NaN): every comparison with it is false, so it enters no count below.  The samples are strided over
//                    the threads; for each of its samples a thread walks the whole image through broadcast LDS reads and counts
//                    the p and y below and equal to its own (the doubled centred average ranks a_i, b_i) and the pairs it wins.
//                    Sums: 64-lane shuffle, one LDS slot per wave, the 4 slots added front to back.  The two arg-max reductions
//                    carry (value, k) and prefer the lower k among equal values, whatever lane holds them.
// No atomics, no arrival counters, no scratch: equal inputs give equal bits, and a row depends on neither the image's place in the
// batch nor on the other images.
//
// Offsets are clamped as fs_ml_image (fs_maploss.hip) clamps them and pixels into [0, value_stride): a malformed table gives wrong
// numbers, never an access outside the buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define FS_MS_THREADS 256
#define FS_MS_WAVES (FS_MS_THREADS / 64)
#define FS_MS_MAX_IMAGE 4096  // labels of one image
#define FS_MS_COLUMNS 12
#define FS_MS_NONE 0x7fffffff  // the k of an arg-max candidate that holds nothing

// [begin, begin + count) of image b, clamped: fs_ml_image's rule
__device__ __forceinline__ void fs_ms_image(const int *__restrict__ d_offsets, int b, int labels, int &begin, int &count) {
    begin = min(max(d_offsets[b], 0), labels);
    int end = min(max(d_offsets[b + 1], begin), labels);
    end = min(end, begin + FS_MS_MAX_IMAGE);
    count = end - begin;
}

__device__ __forceinline__ bool fs_ms_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <typename T>
__device__ __forceinline__ T fs_ms_block_sum(T v, T *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = v;
    __syncthreads();
    T total = slots[0];
#pragma unroll
    for (int w = 1; w < FS_MS_WAVES; ++w) total += slots[w];
    return total;
}

// the better of two arg-max candidates: the larger value, among equal values the lower k; FS_MS_NONE loses to anything
__device__ __forceinline__ void fs_ms_better(float &v, int &k, float ov, int ok) {
    const bool take = ok != FS_MS_NONE && (k == FS_MS_NONE || ov > v || (ov == v && ok < k));
    v = take ? ov : v;
    k = take ? ok : k;
}

// the k of the block's best candidate (-1: nobody holds one)
__device__ __forceinline__ int fs_ms_block_argmax(float v, int k, float *vslots, int *kslots, int tid) {
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(v, off, 64);
        const int ok = __shfl_down(k, off, 64);
        fs_ms_better(v, k, ov, ok);
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        vslots[tid >> 6] = v;
        kslots[tid >> 6] = k;
    }
    __syncthreads();
    v = vslots[0];
    k = kslots[0];
#pragma unroll
    for (int w = 1; w < FS_MS_WAVES; ++w) fs_ms_better(v, k, vslots[w], kslots[w]);
    return k == FS_MS_NONE ? -1 : k;
}

// what sample (pi, yi) counts over the image: the p and y below and equal to its own (itself among the equal), the pairs
// (i, j) it wins and the concordant ones among them.  GAP = false is min_gap == 0, where the double comparison
// (double)yi > (double)yj + 0.0 IS the float comparison.
template <bool GAP>
__device__ __forceinline__ void fs_ms_walk(const float2 *spy, int count, float pi, float yi, double min_gap, int &p_below, int &p_equal,
                                           int &y_below, int &y_equal, int &pairs, int &conc) {
    const double yi_d = (double)yi;
    int pb = 0, pe = 0, yb = 0, ye = 0, won = 0, right = 0;
    for (int j = 0; j < count; ++j) {
        const float2 other = spy[j];  // one address for the whole wave: a broadcast
        const float pj = other.x, yj = other.y;
        pb += pj < pi ? 1 : 0;
        pe += pj == pi ? 1 : 0;
        yb += yj < yi ? 1 : 0;
        ye += yj == yi ? 1 : 0;
        const bool wins = GAP ? yi_d > (double)yj + min_gap : yi > yj;
        won += wins ? 1 : 0;
        right += wins && pi > pj ? 1 : 0;
    }
    p_below = pb, p_equal = pe, y_below = yb, y_equal = ye, pairs = won, conc = right;
}

__global__ __launch_bounds__(FS_MS_THREADS) void fs_k_map_score(const float *__restrict__ d_value, int value_stride,
                                                                 const int *__restrict__ d_pix, const float *__restrict__ d_label,
                                                                 const int *__restrict__ d_offsets, int labels, double min_gap,
                                                                 double *__restrict__ d_rows) {
    __shared__ float2 spy[FS_MS_MAX_IMAGE];  // (p, y) of the image; (NaN, NaN) where the position is not counted
    __shared__ float fslots[FS_MS_WAVES];
    __shared__ int islots[FS_MS_WAVES];
    __shared__ long long lslots[FS_MS_WAVES];
    __shared__ double dslots[FS_MS_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x;
    int begin, count;
    fs_ms_image(d_offsets, b, labels, begin, count);
    const float *value = d_value + (size_t)b * (size_t)value_stride;
    const float nanf_ = __uint_as_float(0x7fc00000u);

    // the image into LDS; per thread, over its samples in rising k: the counted ones, se, and the two arg-max candidates
    int n_part = 0, chosen_k = FS_MS_NONE, best_k = FS_MS_NONE;
    float chosen_v = 0.0f, best_v = 0.0f;
    double se_part = 0.0;
    for (int k = tid; k < count; k += FS_MS_THREADS) {
        const int pix = min(max(d_pix[begin + k], 0), value_stride - 1);
        const float p = value[pix], y = d_label[begin + k];
        const bool counted = fs_ms_finite(p) && fs_ms_finite(y);
        spy[k] = counted ? make_float2(p, y) : make_float2(nanf_, nanf_);
        if (!counted) continue;
        n_part += 1;
        const double diff = (double)p - (double)y;
        se_part += diff * diff;
        fs_ms_better(chosen_v, chosen_k, p, k);
        fs_ms_better(best_v, best_k, y, k);
    }
    __syncthreads();
    const int n = fs_ms_block_sum(n_part, islots, tid);
    const double se = fs_ms_block_sum(se_part, dslots, tid);
    const int chosen = fs_ms_block_argmax(chosen_v, chosen_k, fslots, islots, tid);
    const int best = fs_ms_block_argmax(best_v, best_k, fslots, islots, tid);

    // the walk: per counted sample its doubled centred average ranks a, b and its share of P_b, C_b and of the chosen cell's rank
    const float y_chosen = chosen >= 0 ? spy[chosen].y : nanf_;
    long long sab_part = 0, saa_part = 0, sbb_part = 0;
    int pairs_part = 0, conc_part = 0, above_part = 0;
    for (int i = tid; i < count; i += FS_MS_THREADS) {
        const float pi = spy[i].x, yi = spy[i].y;
        if (pi != pi) continue;  // not counted
        int p_below, p_equal, y_below, y_equal, pairs, conc;
        if (min_gap == 0.0)
            fs_ms_walk<false>(spy, count, pi, yi, min_gap, p_below, p_equal, y_below, y_equal, pairs, conc);
        else
            fs_ms_walk<true>(spy, count, pi, yi, min_gap, p_below, p_equal, y_below, y_equal, pairs, conc);
        const long long a = 2 * p_below + p_equal - n, c = 2 * y_below + y_equal - n;  // 2 rank - (n + 1), |.| <= n
        sab_part += a * c;
        saa_part += a * a;
        sbb_part += c * c;
        pairs_part += pairs;  // <= 16 samples x 4095: fits
        conc_part += conc;
        above_part += yi > y_chosen ? 1 : 0;
    }
    const long long sab = fs_ms_block_sum(sab_part, lslots, tid);
    const long long saa = fs_ms_block_sum(saa_part, lslots, tid);
    const long long sbb = fs_ms_block_sum(sbb_part, lslots, tid);
    const int pairs = fs_ms_block_sum(pairs_part, islots, tid);  // <= 4096 * 4095 / 2: fits
    const int conc = fs_ms_block_sum(conc_part, islots, tid);
    const int above = fs_ms_block_sum(above_part, islots, tid);

    if (tid == 0) {
        const double nan_ = __longlong_as_double(0x7ff8000000000000LL);
        double *row = d_rows + (size_t)b * FS_MS_COLUMNS;
        row[0] = (double)n;
        row[1] = (double)chosen;  // -1 without a counted position
        row[2] = (double)best;
        row[3] = n > 0 ? (double)above : -1.0;
        row[4] = (double)pairs;
        row[5] = (double)conc;
        row[6] = (double)sab;
        row[7] = (double)saa;
        row[8] = (double)sbb;
        row[9] = (n < 2 || saa == 0 || sbb == 0) ? nan_ : (double)sab / sqrt((double)saa * (double)sbb);
        row[10] = n > 0 ? (double)spy[best].y - (double)y_chosen : nan_;
        row[11] = se;
    }
}

extern "C" int fs_map_score(const float *d_value, int value_stride, const int *d_pix, const float *d_label, const int *d_offsets,
                            int images, int labels, double min_gap, double *d_rows, void *stream) {
    if (!d_value || !d_pix || !d_label || !d_offsets || !d_rows) {
        fs_set_error("fs_map_score: null pointer");
        return FS_ERR_ARG;
    }
    for (const void *p : {(const void *)d_value, (const void *)d_pix, (const void *)d_label, (const void *)d_offsets})
        if ((uintptr_t)p % 4) {
            fs_set_error("fs_map_score: float and int pointers must be 4-byte aligned");
            return FS_ERR_ARG;
        }
    if ((uintptr_t)d_rows % 8) {
        fs_set_error("fs_map_score: d_rows must be 8-byte aligned");
        return FS_ERR_ARG;
    }
    if (images < 1 || labels < 1) {
        fs_set_error("fs_map_score: images >= 1 and labels >= 1");
        return FS_ERR_ARG;
    }
    if (value_stride < 1) {
        fs_set_error("fs_map_score: value_stride >= 1");
        return FS_ERR_ARG;
    }
    if (!std::isfinite(min_gap) || min_gap < 0.0) {
        fs_set_error("fs_map_score: min_gap >= 0 and finite");
        return FS_ERR_ARG;
    }
    hipLaunchKernelGGL(fs_k_map_score, dim3(images), dim3(FS_MS_THREADS), 0, (hipStream_t)stream, d_value, value_stride, d_pix,
                       d_label, d_offsets, labels, min_gap, d_rows);
    return fs_hip_ok(hipGetLastError(), "fs_map_score launch") ? FS_OK : FS_ERR_HIP;
}
