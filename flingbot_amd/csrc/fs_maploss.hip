// fs_maploss.hip -- fs_group_loss' rule (squared error + pairwise ranking term, value and gradient) for IMAGES with many labels
// each: any number of images, any total number of labels, normalised per label or per image (flingbot_amd/trainops.py
// MapLossFunction; include/flingsim.h has the rule in full).
//
// fs_k_group_loss is one workgroup: 4096 predictions at the most, and a segment of 4096 keeps one compute unit busy for
// milliseconds.  Here the pairs of an image are found by workgroups of their own, and a long image is split over several:
//   fs_k_map_loss_pairs   grid (image, chunk of 256 samples).  Every workgroup puts ITS image's (p, y) into LDS as float2 (32 KiB
//                         at 4096 labels; the inner loop reads one broadcast 8-byte word per step), every thread walks the image
//                         for its one sample exactly as fs_k_group_loss walks a segment and keeps g_i, its share of the rank sum,
//                         of P_b and of C_b; g_i goes to the work buffer, the four chunk sums (S, R, P, C) -- 64-lane shuffle,
//                         one LDS slot per wave, the 4 slots added front to back -- to the chunk's slot of the work buffer.
//   fs_k_map_loss_finish  up to 128 workgroups.  Each forms the totals by the same fixed schedule (the chunk sums of an image
//                         front to back in fp32, the images strided over the threads in double, the block sum as above), so all
//                         hold the same bits; workgroup w then serves images w, w + 128, ...: their dpred and their table row.
//                         Workgroup 0 writes the statistics.
// No atomics, no arrival counters, nothing read back: equal inputs give equal bits, and what an image contributes (S_b, R_b, P_b,
// C_b, g_i) depends on neither its place in the batch nor on the other images.
//
// Offsets are clamped wherever they are read (fs_ml_image): begin into [0, L], end into [begin, L] and to begin + 4096.  Every
// index below is formed from the clamped values: a malformed table gives wrong numbers, never an access outside the buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"
#include "fs_pair_terms.h"

#define FS_ML_THREADS 256                                   // one chunk: one sample per thread
#define FS_ML_WAVES (FS_ML_THREADS / 64)
#define FS_ML_MAX_IMAGE 4096                                // labels of one image
#define FS_ML_MAX_CHUNKS (FS_ML_MAX_IMAGE / FS_ML_THREADS)  // 16
#define FS_ML_FINISH_GROUPS 128

// the chunk sums of one workgroup of fs_k_map_loss_pairs; slot [image][chunk] of the work buffer
struct fs_ml_partial {
    float sq;    // sum of (p - y)^2
    float rank;  // sum of softplus over the pairs its samples win
    int pairs;
    int conc;
};

// [begin, begin + count) of image b, clamped
__device__ __forceinline__ void fs_ml_image(const int *__restrict__ d_offsets, int b, int labels, int &begin, int &count) {
    begin = min(max(d_offsets[b], 0), labels);
    int end = min(max(d_offsets[b + 1], begin), labels);
    end = min(end, begin + FS_ML_MAX_IMAGE);
    count = end - begin;
}

template <typename T>
__device__ __forceinline__ T fs_ml_block_sum(T v, T *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = v;
    __syncthreads();
    T total = slots[0];
#pragma unroll
    for (int w = 1; w < FS_ML_WAVES; ++w) total += slots[w];
    return total;
}

__global__ __launch_bounds__(FS_ML_THREADS) void fs_k_map_loss_pairs(const float *__restrict__ d_pred,
                                                                      const float *__restrict__ d_label,
                                                                      const int *__restrict__ d_offsets, int labels,
                                                                      double inv_tau, double min_gap,
                                                                      fs_ml_partial *__restrict__ d_partial,
                                                                      float *__restrict__ d_g) {
    __shared__ float2 spy[FS_ML_MAX_IMAGE];  // (p, y) of the image
    __shared__ float fslots[FS_ML_WAVES];
    __shared__ int islots[FS_ML_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x, chunk = blockIdx.y;
    int begin, count;
    fs_ml_image(d_offsets, b, labels, begin, count);
    if (chunk * FS_ML_THREADS >= count) return;  // (uniform: the image has no such chunk, and nobody reads its slot)
    for (int j = tid; j < count; j += FS_ML_THREADS) spy[j] = make_float2(d_pred[begin + j], d_label[begin + j]);
    __syncthreads();

    const int i = chunk * FS_ML_THREADS + tid;
    float g = 0.0f, rank_part = 0.0f, sq_part = 0.0f;  // g: sum over the pairs i loses of sigma, minus the sum over those it wins
    int pairs_part = 0, conc_part = 0;
    if (i < count) {
        const float pi = spy[i].x, yi = spy[i].y;
        const double yi_d = (double)yi, yi_gap = (double)yi + min_gap;
        const float diff = pi - yi;
        sq_part = diff * diff;
        for (int j = 0; j < count; ++j) {
            const float2 other = spy[j];  // one address for the whole wave: a broadcast
            const float pj = other.x, yj = other.y;
            const bool wins = yi_d > (double)yj + min_gap;  // (i, j) is a pair
            const bool loses = (double)yj > yi_gap;          // (j, i) is a pair
            if (!wins && !loses) continue;
            // the winner's margin in the prediction; x = -margin / tau
            const double margin = wins ? (double)pi - (double)pj : (double)pj - (double)pi;
            const fs_pair_terms t = fs_pair_eval(margin, inv_tau);
            if (wins) {
                rank_part += fs_pair_softplus(t);
                g -= t.sig;
                pairs_part += 1;
                conc_part += margin > 0.0 ? 1 : 0;
            } else {
                g += t.sig;
            }
        }
        d_g[begin + i] = g;
    }
    const float sq_sum = fs_ml_block_sum(sq_part, fslots, tid);
    const float rank_sum = fs_ml_block_sum(rank_part, fslots, tid);
    const int pairs = fs_ml_block_sum(pairs_part, islots, tid);
    const int conc = fs_ml_block_sum(conc_part, islots, tid);
    if (tid == 0) {
        fs_ml_partial out;
        out.sq = sq_sum;
        out.rank = rank_sum;
        out.pairs = pairs;
        out.conc = conc;
        d_partial[(size_t)b * FS_ML_MAX_CHUNKS + chunk] = out;
    }
}

// S_b, R_b, P_b, C_b: the chunk sums of image b (count labels) front to back
__device__ __forceinline__ fs_ml_partial fs_ml_image_sums(const fs_ml_partial *__restrict__ d_partial, int b, int count) {
    fs_ml_partial sum = {0.0f, 0.0f, 0, 0};
    const int chunks = (count + FS_ML_THREADS - 1) / FS_ML_THREADS;  // <= 16 by the clamp
    for (int c = 0; c < chunks; ++c) {
        const fs_ml_partial part = d_partial[(size_t)b * FS_ML_MAX_CHUNKS + c];
        sum.sq += part.sq;
        sum.rank += part.rank;
        sum.pairs += part.pairs;  // <= 4096 * 4095 / 2: fits
        sum.conc += part.conc;
    }
    return sum;
}

__global__ __launch_bounds__(FS_ML_THREADS) void fs_k_map_loss_finish(const float *__restrict__ d_pred,
                                                                       const float *__restrict__ d_label,
                                                                       const int *__restrict__ d_offsets, int images, int labels,
                                                                       double weight, double inv_tau, int per_image, float scale,
                                                                       const fs_ml_partial *__restrict__ d_partial,
                                                                       const float *__restrict__ d_g, float *__restrict__ d_dpred,
                                                                       double *__restrict__ d_stats, float *__restrict__ d_table) {
    __shared__ double dslots[FS_ML_WAVES];
    __shared__ long long lslots[FS_ML_WAVES];
    const int tid = threadIdx.x;
    // the totals: every workgroup forms them alike
    double sq_acc = 0.0, rank_acc = 0.0;
    long long pairs_acc = 0, conc_acc = 0, filled_acc = 0, ranked_acc = 0;
    for (int b = tid; b < images; b += FS_ML_THREADS) {
        int begin, count;
        fs_ml_image(d_offsets, b, labels, begin, count);
        if (count == 0) continue;
        const fs_ml_partial sum = fs_ml_image_sums(d_partial, b, count);
        sq_acc += per_image ? (double)(sum.sq / (float)count) : (double)sum.sq;
        if (sum.pairs > 0) rank_acc += per_image ? (double)(sum.rank / (float)sum.pairs) : (double)sum.rank;
        pairs_acc += sum.pairs;
        conc_acc += sum.conc;
        filled_acc += 1;
        ranked_acc += sum.pairs > 0 ? 1 : 0;
    }
    const double sq_total = fs_ml_block_sum(sq_acc, dslots, tid);
    const double rank_total = fs_ml_block_sum(rank_acc, dslots, tid);
    const long long pairs = fs_ml_block_sum(pairs_acc, lslots, tid);
    const long long conc = fs_ml_block_sum(conc_acc, lslots, tid);
    const long long filled = fs_ml_block_sum(filled_acc, lslots, tid);   // G'
    const long long ranked = fs_ml_block_sum(ranked_acc, lslots, tid);   // G''

    if (blockIdx.x == 0 && tid == 0) {
        const double mse = per_image ? (filled > 0 ? sq_total / (double)filled : 0.0) : sq_total / (double)labels;
        const double rank = pairs > 0 ? rank_total / (double)(per_image ? ranked : pairs) : 0.0;
        d_stats[0] = mse + weight * rank;
        d_stats[1] = mse;
        d_stats[2] = rank;
        d_stats[3] = (double)pairs;
        d_stats[4] = (double)conc;
        d_stats[5] = (double)filled;
        d_stats[6] = (double)ranked;
        d_stats[7] = 0.0;
    }

    const float fl = (float)labels;
    for (int b = blockIdx.x; b < images; b += gridDim.x) {
        int begin, count;
        fs_ml_image(d_offsets, b, labels, begin, count);
        const fs_ml_partial sum = fs_ml_image_sums(d_partial, b, count);  // (count = 0: zeros)
        if (tid == 0) {
            d_table[4 * (size_t)b + 0] = count > 0 ? sum.sq / (float)count : 0.0f;
            d_table[4 * (size_t)b + 1] = sum.pairs > 0 ? sum.rank / (float)sum.pairs : 0.0f;
            d_table[4 * (size_t)b + 2] = (float)sum.pairs;  // <= 4096 * 4095 / 2 < 2^24: exact
            d_table[4 * (size_t)b + 3] = (float)sum.conc;
        }
        // without pairs in the image (or weight) the second term is ABSENT, not 0 * something
        const bool with_rank = sum.pairs > 0 && weight > 0.0;
        const float denom = per_image ? (float)((double)filled * (double)count) : fl;
        const float coef = !with_rank ? 0.0f
                           : per_image ? (float)(weight * inv_tau / ((double)ranked * (double)sum.pairs))
                                       : (float)(weight * inv_tau / (double)pairs);
        for (int i = tid; i < count; i += FS_ML_THREADS) {
            float d = 2.0f * (d_pred[begin + i] - d_label[begin + i]) / denom;
            if (with_rank) d = d + coef * d_g[begin + i];
            d_dpred[begin + i] = scale * d;
        }
    }
}

static bool fs_ml_served(int images, int labels) { return images >= 1 && labels >= 1; }

extern "C" size_t fs_map_loss_work_bytes(int images, int labels) {
    if (!fs_ml_served(images, labels)) return 0;
    return (size_t)images * FS_ML_MAX_CHUNKS * sizeof(fs_ml_partial) + (size_t)labels * sizeof(float);
}

extern "C" int fs_map_loss(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels, double weight,
                           double temperature, double min_gap, int per_image, double grad_scale, float *d_dpred, double *d_stats,
                           float *d_table, void *d_work, void *stream) {
    if (!d_pred || !d_label || !d_offsets || !d_dpred || !d_stats || !d_table || !d_work) {
        fs_set_error("fs_map_loss: null pointer");
        return FS_ERR_ARG;
    }
    for (const void *p : {(const void *)d_pred, (const void *)d_label, (const void *)d_offsets, (const void *)d_dpred,
                          (const void *)d_table})
        if ((uintptr_t)p % 4) {
            fs_set_error("fs_map_loss: float and int pointers must be 4-byte aligned");
            return FS_ERR_ARG;
        }
    if ((uintptr_t)d_stats % 8 || (uintptr_t)d_work % 8) {
        fs_set_error("fs_map_loss: d_stats and d_work must be 8-byte aligned");
        return FS_ERR_ARG;
    }
    if (!fs_ml_served(images, labels)) {
        fs_set_error("fs_map_loss: images >= 1 and labels >= 1");
        return FS_ERR_ARG;
    }
    if (per_image != 0 && per_image != 1) {
        fs_set_error("fs_map_loss: per_image is 0 or 1");
        return FS_ERR_ARG;
    }
    if (!std::isfinite(weight) || weight < 0.0 || !std::isfinite(temperature) || temperature <= 0.0 || !std::isfinite(min_gap) ||
        min_gap < 0.0 || !std::isfinite(grad_scale) || !std::isfinite((float)grad_scale) || !std::isfinite((float)weight) ||
        !std::isfinite(1.0 / temperature)) {
        fs_set_error("fs_map_loss: weight >= 0, temperature > 0, min_gap >= 0 and grad_scale must be finite");
        return FS_ERR_ARG;
    }
    fs_ml_partial *d_partial = (fs_ml_partial *)d_work;
    float *d_g = (float *)(d_partial + (size_t)images * FS_ML_MAX_CHUNKS);
    const double inv_tau = 1.0 / temperature;
    const int longest = labels < FS_ML_MAX_IMAGE ? labels : FS_ML_MAX_IMAGE;  // no image has more labels than this
    const int chunks = (longest + FS_ML_THREADS - 1) / FS_ML_THREADS;
    // (image, chunk): the images along x, whose limit is 2^31 - 1
    hipLaunchKernelGGL(fs_k_map_loss_pairs, dim3(images, chunks), dim3(FS_ML_THREADS), 0, (hipStream_t)stream, d_pred, d_label,
                       d_offsets, labels, inv_tau, min_gap, d_partial, d_g);
    if (!fs_hip_ok(hipGetLastError(), "fs_map_loss pairs launch")) return FS_ERR_HIP;
    const int groups = images < FS_ML_FINISH_GROUPS ? images : FS_ML_FINISH_GROUPS;
    hipLaunchKernelGGL(fs_k_map_loss_finish, dim3(groups), dim3(FS_ML_THREADS), 0, (hipStream_t)stream, d_pred, d_label, d_offsets,
                       images, labels, weight, inv_tau, per_image, (float)grad_scale, d_partial, d_g, d_dpred, d_stats, d_table);
    return fs_hip_ok(hipGetLastError(), "fs_map_loss finish launch") ? FS_OK : FS_ERR_HIP;
}
