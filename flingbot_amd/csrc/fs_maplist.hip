// fs_maplist.hip -- the LISTWISE term over images with many labels each: per image the KL divergence between the Boltzmann
// distribution of the labels and that of the predictions (ListNet's top-one cross-entropy), value and gradient, for any number of
// images and any total number of labels, normalised per label or per image (flingbot_amd/trainops.py MapListFunction;
// include/flingsim.h has the rule in full).  O(K) per image, where fs_map_loss' pair walk is O(K^2).
//
//   fs_k_map_list_image   one workgroup per image.  Thread t holds labels t, t + 256, ... of the image -- at most 16 -- as doubles
//                         a = p / T_p and c = y / T_y in registers; a slot the image does not reach costs one uniform branch, so
//                         an image of 144 labels runs one slot and one of 4096 all sixteen.  Five block reductions (64-lane
//                         shuffle, one LDS slot per wave, the 4 slots front to back): the arg-max of p and of y as (value, index)
//                         pairs, the two sums of exp below the maximum, and D_b.  g_i (double, not yet normalised) and the
//                         image's record go to the work buffer, the table row to d_table.
//   fs_k_map_list_finish  up to 128 workgroups.  Each forms G_l, L_l and the totals by the same fixed schedule (the images strided
//                         over the threads in double, then the block sum as above), so all hold the same bits; workgroup w then
//                         writes d_dpred for images w, w + 128, ...  Workgroup 0 writes the statistics.
// No atomics, no arrival counters, nothing read back: equal inputs give equal bits, and what an image contributes (D_b, g_i, its
// table row) depends on neither its place in the batch nor on the other images.  The arg-max order -- larger value first, then
// lower index, NaN below everything -- is total, so the winner does not depend on the shape of the reduction tree.
//
// log-softmax with the maximum's own addend taken out of the sum: with m the arg-max,  log sum_j exp(a_j - a_m) =
// log1p(sum_{j != m} exp(a_j - a_m)),  and  ls_i = (a_i - a_m) - log1p(..): two terms of one sign, so no cancellation however
// peaked the distribution is, and nothing overflows or turns into -inf for finite inputs.
//
// Offsets are clamped wherever they are read (fs_ll_image, fs_ml_image's rule): begin into [0, L], end into [begin, L] and to
// begin + 4096.  Every index below is formed from the clamped values: a malformed table gives wrong numbers, never an access
// outside the buffers.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define FS_LL_THREADS 256
#define FS_LL_WAVES (FS_LL_THREADS / 64)
#define FS_LL_MAX_IMAGE 4096                             // labels of one image
#define FS_LL_SLOTS (FS_LL_MAX_IMAGE / FS_LL_THREADS)    // 16 labels per thread at the most
#define FS_LL_FINISH_GROUPS 128

// what fs_k_map_list_image leaves for the finish kernel; slot [image] of the work buffer
struct fs_ll_record {
    double kl;        // D_b
    double q_chosen;  // q at the arg-max of p
    double q_best;    // max q
    int chosen;       // the arg-max of p, within the image
    int best;         // the arg-max of y
};

struct fs_ll_top {
    float v;
    int k;
};

// [begin, begin + count) of image b, clamped
__device__ __forceinline__ void fs_ll_image(const int *__restrict__ d_offsets, int b, int labels, int &begin, int &count) {
    begin = min(max(d_offsets[b], 0), labels);
    int end = min(max(d_offsets[b + 1], begin), labels);
    end = min(end, begin + FS_LL_MAX_IMAGE);
    count = end - begin;
}

// the larger value, among equals the lower index (v is never NaN here: a total order)
__device__ __forceinline__ fs_ll_top fs_ll_better(fs_ll_top a, fs_ll_top b) {
    return (b.v > a.v || (b.v == a.v && b.k < a.k)) ? b : a;
}

__device__ __forceinline__ fs_ll_top fs_ll_block_top(fs_ll_top t, fs_ll_top *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) {
        fs_ll_top other;
        other.v = __shfl_down(t.v, off, 64);
        other.k = __shfl_down(t.k, off, 64);
        t = fs_ll_better(t, other);
    }
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = t;
    __syncthreads();
    fs_ll_top best = slots[0];
#pragma unroll
    for (int w = 1; w < FS_LL_WAVES; ++w) best = fs_ll_better(best, slots[w]);
    return best;
}

template <typename T>
__device__ __forceinline__ T fs_ll_block_sum(T v, T *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = v;
    __syncthreads();
    T total = slots[0];
#pragma unroll
    for (int w = 1; w < FS_LL_WAVES; ++w) total += slots[w];
    return total;
}

__global__ __launch_bounds__(FS_LL_THREADS) void fs_k_map_list_image(const float *__restrict__ d_pred,
                                                                      const float *__restrict__ d_label,
                                                                      const int *__restrict__ d_offsets, int labels,
                                                                      double pred_temperature, double label_temperature,
                                                                      fs_ll_record *__restrict__ d_record,
                                                                      double *__restrict__ d_g, float *__restrict__ d_table) {
    __shared__ fs_ll_top tslots[FS_LL_WAVES];
    __shared__ double dslots[FS_LL_WAVES];
    __shared__ double q_chosen;
    const int tid = threadIdx.x, b = blockIdx.x;
    int begin, count;
    fs_ll_image(d_offsets, b, labels, begin, count);
    if (count < 2) {  // (uniform) not listed: nobody reads its record or its g
        if (tid == 0) {
            d_table[4 * (size_t)b + 0] = 0.0f;
            d_table[4 * (size_t)b + 1] = 0.0f;
            d_table[4 * (size_t)b + 2] = -1.0f;
            d_table[4 * (size_t)b + 3] = -1.0f;
        }
        return;
    }

    double a[FS_LL_SLOTS], c[FS_LL_SLOTS];
    fs_ll_top top_p = {-INFINITY, INT_MAX}, top_y = {-INFINITY, INT_MAX};
#pragma unroll
    for (int k = 0; k < FS_LL_SLOTS; ++k) {
        a[k] = 0.0;
        c[k] = 0.0;
        if (k * FS_LL_THREADS < count) {  // (uniform)
            const int i = k * FS_LL_THREADS + tid;
            if (i < count) {
                const float p = d_pred[begin + i], y = d_label[begin + i];
                a[k] = (double)p / pred_temperature;
                c[k] = (double)y / label_temperature;
                const fs_ll_top cand_p = {p != p ? -INFINITY : p, i}, cand_y = {y != y ? -INFINITY : y, i};  // NaN never wins
                top_p = fs_ll_better(top_p, cand_p);
                top_y = fs_ll_better(top_y, cand_y);
            }
        }
    }
    top_p = fs_ll_block_top(top_p, tslots, tid);  // index 0 exists, so .k lies in [0, count)
    top_y = fs_ll_block_top(top_y, tslots, tid);
    const double max_a = (double)top_p.v / pred_temperature, max_c = (double)top_y.v / label_temperature;

    double za = 0.0, zc = 0.0;  // the sums of exp without the maximum's own 1
#pragma unroll
    for (int k = 0; k < FS_LL_SLOTS; ++k) {
        if (k * FS_LL_THREADS < count) {
            const int i = k * FS_LL_THREADS + tid;
            if (i < count) {
                if (i != top_p.k) za += exp(a[k] - max_a);
                if (i != top_y.k) zc += exp(c[k] - max_c);
            }
        }
    }
    const double log_za = log1p(fs_ll_block_sum(za, dslots, tid));
    const double log_zc = log1p(fs_ll_block_sum(zc, dslots, tid));

    double kl = 0.0;
#pragma unroll
    for (int k = 0; k < FS_LL_SLOTS; ++k) {
        if (k * FS_LL_THREADS < count) {
            const int i = k * FS_LL_THREADS + tid;
            if (i < count) {
                const double ls = (a[k] - max_a) - log_za, lq = (c[k] - max_c) - log_zc;
                const double s = exp(ls), q = exp(lq);
                kl += q == 0.0 ? 0.0 : q * (lq - ls);  // an underflowed q contributes exactly 0
                d_g[begin + i] = (s - q) / pred_temperature;
                if (i == top_p.k) q_chosen = q;  // (one thread; read after the barriers of the sum below)
            }
        }
    }
    kl = fs_ll_block_sum(kl, dslots, tid);
    if (tid == 0) {
        fs_ll_record out;
        out.kl = kl;
        out.q_chosen = q_chosen;
        out.q_best = exp(0.0 - log_zc);  // lq at the arg-max of y: (c - max_c) is +0.0 there
        out.chosen = top_p.k;
        out.best = top_y.k;
        d_record[b] = out;
        d_table[4 * (size_t)b + 0] = (float)kl;
        d_table[4 * (size_t)b + 1] = (float)q_chosen;
        d_table[4 * (size_t)b + 2] = (float)top_p.k;  // < 4096: exact
        d_table[4 * (size_t)b + 3] = (float)top_y.k;
    }
}

__global__ __launch_bounds__(FS_LL_THREADS) void fs_k_map_list_finish(const int *__restrict__ d_offsets, int images, int labels,
                                                                       double weight, int per_image, double grad_scale,
                                                                       const fs_ll_record *__restrict__ d_record,
                                                                       const double *__restrict__ d_g,
                                                                       float *__restrict__ d_dpred, double *__restrict__ d_stats) {
    __shared__ double dslots[FS_LL_WAVES];
    __shared__ long long lslots[FS_LL_WAVES];
    const int tid = threadIdx.x;
    // the totals: every workgroup forms them alike
    double kl_acc = 0.0, chosen_acc = 0.0, best_acc = 0.0;
    long long listed_acc = 0, labels_acc = 0, hits_acc = 0;
    for (int b = tid; b < images; b += FS_LL_THREADS) {
        int begin, count;
        fs_ll_image(d_offsets, b, labels, begin, count);
        if (count < 2) continue;
        const fs_ll_record rec = d_record[b];
        kl_acc += per_image ? rec.kl : (double)count * rec.kl;
        chosen_acc += rec.q_chosen;
        best_acc += rec.q_best;
        listed_acc += 1;
        labels_acc += count;
        hits_acc += rec.chosen == rec.best ? 1 : 0;
    }
    const double kl_total = fs_ll_block_sum(kl_acc, dslots, tid);
    const double chosen_total = fs_ll_block_sum(chosen_acc, dslots, tid);
    const double best_total = fs_ll_block_sum(best_acc, dslots, tid);
    const long long listed = fs_ll_block_sum(listed_acc, lslots, tid);        // G_l
    const long long listed_labels = fs_ll_block_sum(labels_acc, lslots, tid);  // L_l
    const long long hits = fs_ll_block_sum(hits_acc, lslots, tid);             // H

    if (blockIdx.x == 0 && tid == 0) {
        const double list = listed > 0 ? kl_total / (double)(per_image ? listed : listed_labels) : 0.0;
        d_stats[0] = weight * list;
        d_stats[1] = list;
        d_stats[2] = (double)listed;
        d_stats[3] = (double)listed_labels;
        d_stats[4] = (double)hits;
        d_stats[5] = listed > 0 ? chosen_total / (double)listed : 0.0;
        d_stats[6] = listed > 0 ? best_total / (double)listed : 0.0;
        d_stats[7] = 0.0;
    }

    const double scale = grad_scale * weight;
    for (int b = blockIdx.x; b < images; b += gridDim.x) {
        int begin, count;
        fs_ll_image(d_offsets, b, labels, begin, count);
        if (count < 2 || weight == 0.0) {  // not listed, or no term at all: zeros, whatever g holds
            for (int i = tid; i < count; i += FS_LL_THREADS) d_dpred[begin + i] = 0.0f;
            continue;
        }
        const double coef = per_image ? 1.0 / (double)listed : (double)count / (double)listed_labels;
        const double factor = scale * coef;
        for (int i = tid; i < count; i += FS_LL_THREADS) d_dpred[begin + i] = (float)(factor * d_g[begin + i]);
    }
}

static bool fs_ll_served(int images, int labels) { return images >= 1 && labels >= 1; }

extern "C" size_t fs_map_list_work_bytes(int images, int labels) {
    if (!fs_ll_served(images, labels)) return 0;
    return (size_t)images * sizeof(fs_ll_record) + (size_t)labels * sizeof(double);
}

extern "C" int fs_map_list_loss(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels,
                                double weight, double pred_temperature, double label_temperature, int per_image,
                                double grad_scale, float *d_dpred, double *d_stats, float *d_table, void *d_work, void *stream) {
    if (!d_pred || !d_label || !d_offsets || !d_dpred || !d_stats || !d_table || !d_work) {
        fs_set_error("fs_map_list_loss: null pointer");
        return FS_ERR_ARG;
    }
    for (const void *p : {(const void *)d_pred, (const void *)d_label, (const void *)d_offsets, (const void *)d_dpred,
                          (const void *)d_table})
        if ((uintptr_t)p % 4) {
            fs_set_error("fs_map_list_loss: float and int pointers must be 4-byte aligned");
            return FS_ERR_ARG;
        }
    if ((uintptr_t)d_stats % 8 || (uintptr_t)d_work % 8) {
        fs_set_error("fs_map_list_loss: d_stats and d_work must be 8-byte aligned");
        return FS_ERR_ARG;
    }
    if (!fs_ll_served(images, labels)) {
        fs_set_error("fs_map_list_loss: images >= 1 and labels >= 1");
        return FS_ERR_ARG;
    }
    if (per_image != 0 && per_image != 1) {
        fs_set_error("fs_map_list_loss: per_image is 0 or 1");
        return FS_ERR_ARG;
    }
    if (!std::isfinite(weight) || weight < 0.0 || !std::isfinite((float)weight) || !std::isfinite(pred_temperature) ||
        pred_temperature <= 0.0 || !std::isfinite(1.0 / pred_temperature) || !std::isfinite((float)pred_temperature) ||
        !std::isfinite(label_temperature) || label_temperature <= 0.0 || !std::isfinite(1.0 / label_temperature) ||
        !std::isfinite((float)label_temperature) || !std::isfinite(grad_scale) || !std::isfinite((float)grad_scale)) {
        fs_set_error("fs_map_list_loss: weight >= 0, both temperatures > 0 with finite reciprocals, and grad_scale must be finite");
        return FS_ERR_ARG;
    }
    static_assert(sizeof(fs_ll_record) % 8 == 0, "g follows the records as doubles");
    fs_ll_record *d_record = (fs_ll_record *)d_work;
    double *d_g = (double *)(d_record + (size_t)images);
    hipLaunchKernelGGL(fs_k_map_list_image, dim3(images), dim3(FS_LL_THREADS), 0, (hipStream_t)stream, d_pred, d_label, d_offsets,
                       labels, pred_temperature, label_temperature, d_record, d_g, d_table);
    if (!fs_hip_ok(hipGetLastError(), "fs_map_list_loss image launch")) return FS_ERR_HIP;
    const int groups = images < FS_LL_FINISH_GROUPS ? images : FS_LL_FINISH_GROUPS;
    hipLaunchKernelGGL(fs_k_map_list_finish, dim3(groups), dim3(FS_LL_THREADS), 0, (hipStream_t)stream, d_offsets, images, labels,
                       weight, per_image, grad_scale, d_record, d_g, d_dpred, d_stats);
    return fs_hip_ok(hipGetLastError(), "fs_map_list_loss finish launch") ? FS_OK : FS_ERR_HIP;
}
