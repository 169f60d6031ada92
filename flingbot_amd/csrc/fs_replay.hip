// fs_replay.hip -- one training batch out of a device-resident replay buffer (flingbot_amd/replay.py ExperienceSet).
//
// Reference: learning/utils.py GraspDataset.__getitem__ (:76-100) -- per sample: read observation, action mask and the
// coverage attributes, select channels and, in rgb_only mode, push the image through
// ToPILImage -> torchvision ColorJitter(0.2, 0.3, 0.5, 0.5) -> ToTensor on the host.  For PIL inputs that jitter is a
// chain of Pillow calls: ImageEnhance.Brightness / Contrast / Color (Image.blend with a degenerate image, Blend.c) and an
// RGB -> HSV -> RGB round trip with the H plane shifted (Convert.c rgb2hsv_row / hsv2rgb), in a per-sample random order.
//
// Here: ONE launch per batch, one workgroup of 256 threads per sample.  The 64 x 64 image is quantised into LDS (one
// packed RGB dword per pixel, 16 KiB) and stays there across the four operations; HBM is read once and written once.
// The arithmetic restates Pillow's, type for type, so that the result is bit-identical to it (replay.py
// color_jitter_host is the numpy form of the same statements, pinned to Pillow by tests/golden/jitter_golden.npz):
//   L            (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   blend        trunc(clip(d + a * (x - d), 0, 255)), product and sum each rounded to fp32 (-ffp-contract=off)
//   degenerate   black (brightness), L (saturation), int(mean(L) + 0.5) of the image as it stands (contrast; the mean
//                is an exact integer block reduction, divided in double)
//   RGB -> HSV   s and the per-channel ratios in float, the hue term and fmod(h / 6 + 1, 1) in double, every assignment
//                to Pillow's `float h` rounding to float
//   hue shift    (int)(h * 255) in double, truncated toward zero, mod 256, added to the uint8 hue with wrap-around
//   HSV -> RGB   in double, p / q / t rounded half away from zero
// The float quotients of two integers below 256 are formed as (float)((double)a / (double)b): the double quotient is
// never within 2^-53 (relative) of a float rounding boundary unless it is exact, so this IS the correctly rounded float
// quotient whatever the compiler's fp32 division expands to.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define FS_REPLAY_DIM 64
#define FS_REPLAY_PIXELS (FS_REPLAY_DIM * FS_REPLAY_DIM)
#define FS_REPLAY_THREADS 256
#define FS_REPLAY_TABLE 9  // ints per sample: index, the four operations in order, the four factors' bits

__device__ __forceinline__ float fs_ratio(int a, int b) { return (float)((double)a / (double)b); }

__device__ __forceinline__ int fs_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int fs_blend(int d, int x, float a) {
    const float prod = a * (float)(x - d);
    float t = (float)d + prod;
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (int)t;
}

__device__ __forceinline__ int fs_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ uint32_t fs_pack(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

// Convert.c rgb2hsv_row, then the wrap-around hue shift, then Convert.c hsv2rgb
__device__ __forceinline__ uint32_t fs_hue_pixel(uint32_t px, int shift) {
    const int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int v = maxc;
    if (minc != maxc) {
        const int cr = maxc - minc;
        const float s = fs_ratio(cr, maxc);
        const float rc = fs_ratio(maxc - r, cr), gc = fs_ratio(maxc - g, cr), bc = fs_ratio(maxc - b, cr);
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double turn = (double)h / 6.0 + 1.0;  // in [5/6, 11/6): fmod(turn, 1.0) == turn - floor(turn), exactly
        h = (float)(turn - floor(turn));
        uh = fs_clip8((int)((double)h * 255.0));
        us = fs_clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) return fs_pack(v, v, v);
    const double x6 = (double)uh * 6.0 / 255.0;
    const double fl = floor(x6);
    const double f = (double)(float)(x6 - fl);
    const double fs = (double)(float)((double)us / 255.0);
    const double vd = (double)v;
    const int p = fs_clip8((int)round(vd * (1.0 - fs)));
    const int q = fs_clip8((int)round(vd * (1.0 - fs * f)));
    const int t = fs_clip8((int)round(vd * (1.0 - fs * (1.0 - f))));
    switch ((int)fl % 6) {
        case 0: return fs_pack(v, t, p);
        case 1: return fs_pack(q, v, p);
        case 2: return fs_pack(p, v, t);
        case 3: return fs_pack(p, q, v);
        case 4: return fs_pack(t, p, v);
        default: return fs_pack(v, p, q);
    }
}

// table[s] = {index, op0..op3, bits of the brightness / contrast / saturation / hue factors}
// d_obs [n][4][64][64], d_masks [n][64][64] bytes, d_labels [n]; out_obs [batch][c_cnt][64][64]
__global__ __launch_bounds__(FS_REPLAY_THREADS) void fs_k_replay_sample(
    const float *__restrict__ d_obs, const unsigned char *__restrict__ d_masks, const float *__restrict__ d_labels, int n,
    const int *__restrict__ table, int c_off, int c_cnt, int jitter, float *__restrict__ out_obs,
    unsigned char *__restrict__ out_mask, float *__restrict__ out_label) {
    __shared__ uint32_t img[FS_REPLAY_PIXELS];
    __shared__ int wave_sum[FS_REPLAY_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int *row = table + (size_t)s * FS_REPLAY_TABLE;
    const int idx = row[0];
    if ((unsigned)idx >= (unsigned)n) return;  // (the host checks the indices; nothing outside the set is ever read)
    const float *src = d_obs + ((size_t)idx * 4 + c_off) * FS_REPLAY_PIXELS;
    float *dst = out_obs + (size_t)s * c_cnt * FS_REPLAY_PIXELS;
    // mask: 4096 bytes, 16 per thread; label
    reinterpret_cast<uint4 *>(out_mask + (size_t)s * FS_REPLAY_PIXELS)[tid] =
        reinterpret_cast<const uint4 *>(d_masks + (size_t)idx * FS_REPLAY_PIXELS)[tid];
    if (tid == 0) out_label[s] = d_labels[idx];
    if (!jitter) {  // the recorded floats, unchanged
        for (int q = tid; q < c_cnt * (FS_REPLAY_PIXELS / 4); q += FS_REPLAY_THREADS)
            reinterpret_cast<float4 *>(dst)[q] = reinterpret_cast<const float4 *>(src)[q];
        return;
    }
    // quantise: trunc(clamp(x * 255, 0, 255)); thread t holds pixels 4 (t + 256 k) .. + 3
    for (int k = 0; k < FS_REPLAY_PIXELS / (4 * FS_REPLAY_THREADS); ++k) {
        const int q = tid + FS_REPLAY_THREADS * k;
        const float4 cr = reinterpret_cast<const float4 *>(src)[q];
        const float4 cg = reinterpret_cast<const float4 *>(src + FS_REPLAY_PIXELS)[q];
        const float4 cb = reinterpret_cast<const float4 *>(src + 2 * FS_REPLAY_PIXELS)[q];
        const float rr[4] = {cr.x, cr.y, cr.z, cr.w}, gg[4] = {cg.x, cg.y, cg.z, cg.w}, bb[4] = {cb.x, cb.y, cb.z, cb.w};
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (int)fminf(fmaxf(rr[j] * 255.0f, 0.0f), 255.0f);
            const int g = (int)fminf(fmaxf(gg[j] * 255.0f, 0.0f), 255.0f);
            const int b = (int)fminf(fmaxf(bb[j] * 255.0f, 0.0f), 255.0f);
            px[j] = fs_pack(r, g, b);
        }
        reinterpret_cast<uint4 *>(img)[q] = make_uint4(px[0], px[1], px[2], px[3]);
    }
    // every thread works on the pixels it wrote itself (dwords 4 q .. 4 q + 3 of its own uint4s): the only exchange
    // between threads is the contrast sum
    for (int stage = 0; stage < 4; ++stage) {
        const int op = row[1 + stage];
        const float a = __int_as_float(row[5 + (op & 3)]);
        if (op == 1) {  // contrast: the mean of L over the image as it stands (block-uniform branch)
            int part = 0;
            for (int k = 0; k < FS_REPLAY_PIXELS / (4 * FS_REPLAY_THREADS); ++k) {
                const uint4 v = reinterpret_cast<const uint4 *>(img)[tid + FS_REPLAY_THREADS * k];
                const uint32_t px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) part += fs_luma(px[j] & 255, (px[j] >> 8) & 255, (px[j] >> 16) & 255);
            }
            for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
            __syncthreads();  // (a second contrast stage cannot exist, but wave_sum's readers of any earlier use are done)
            if ((tid & 63) == 0) wave_sum[tid >> 6] = part;
            __syncthreads();
            int total = 0;
#pragma unroll
            for (int w = 0; w < FS_REPLAY_THREADS / 64; ++w) total += wave_sum[w];  // <= 4096 * 255: exact
            const int mean = (int)((double)total / (double)FS_REPLAY_PIXELS + 0.5);
            for (int k = 0; k < FS_REPLAY_PIXELS / (4 * FS_REPLAY_THREADS); ++k) {
                uint4 v = reinterpret_cast<uint4 *>(img)[tid + FS_REPLAY_THREADS * k];
                uint32_t px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    px[j] = fs_pack(fs_blend(mean, px[j] & 255, a), fs_blend(mean, (px[j] >> 8) & 255, a),
                                    fs_blend(mean, (px[j] >> 16) & 255, a));
                reinterpret_cast<uint4 *>(img)[tid + FS_REPLAY_THREADS * k] = make_uint4(px[0], px[1], px[2], px[3]);
            }
        } else {
            const int shift = (int)((double)a * 255.0) & 255;  // hue: C truncation, then mod 256 (two's complement)
            for (int k = 0; k < FS_REPLAY_PIXELS / (4 * FS_REPLAY_THREADS); ++k) {
                uint4 v = reinterpret_cast<uint4 *>(img)[tid + FS_REPLAY_THREADS * k];
                uint32_t px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = px[j] & 255, g = (px[j] >> 8) & 255, b = (px[j] >> 16) & 255;
                    if (op == 0) {
                        px[j] = fs_pack(fs_blend(0, r, a), fs_blend(0, g, a), fs_blend(0, b, a));
                    } else if (op == 2) {
                        const int l = fs_luma(r, g, b);
                        px[j] = fs_pack(fs_blend(l, r, a), fs_blend(l, g, a), fs_blend(l, b, a));
                    } else {
                        px[j] = fs_hue_pixel(px[j], shift);
                    }
                }
                reinterpret_cast<uint4 *>(img)[tid + FS_REPLAY_THREADS * k] = make_uint4(px[0], px[1], px[2], px[3]);
            }
        }
    }
    // ToTensor: uint8 / 255 in float
    for (int k = 0; k < FS_REPLAY_PIXELS / (4 * FS_REPLAY_THREADS); ++k) {
        const int q = tid + FS_REPLAY_THREADS * k;
        const uint4 v = reinterpret_cast<const uint4 *>(img)[q];
        const uint32_t px[4] = {v.x, v.y, v.z, v.w};
        float o[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[0][j] = fs_ratio(px[j] & 255, 255);
            o[1][j] = fs_ratio((px[j] >> 8) & 255, 255);
            o[2][j] = fs_ratio((px[j] >> 16) & 255, 255);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            reinterpret_cast<float4 *>(dst + c * FS_REPLAY_PIXELS)[q] = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    }
}

extern "C" int fs_replay_sample(const float *d_obs, const unsigned char *d_masks, const float *d_labels, int n_samples,
                                const int *d_table, int batch, int channel_offset, int channels, int jitter, int size,
                                float *d_out_obs, unsigned char *d_out_mask, float *d_out_label, void *stream) {
    if (!d_obs || !d_masks || !d_labels || !d_table || !d_out_obs || !d_out_mask || !d_out_label || n_samples <= 0 ||
        batch <= 0 || channel_offset < 0 || channels <= 0 || channel_offset + channels > 4) {
        fs_set_error("fs_replay_sample: bad arguments");
        return FS_ERR_ARG;
    }
    if (size != FS_REPLAY_DIM) {
        fs_set_error("fs_replay_sample: observations of 64 x 64 pixels only");
        return FS_ERR_ARG;
    }
    if (jitter && (channel_offset != 0 || channels != 3)) {
        fs_set_error("fs_replay_sample: the colour jitter applies to the three colour channels (rgb_only) only");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_obs, d_masks, d_out_obs, d_out_mask})) {
        fs_set_error("fs_replay_sample: buffers must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    hipLaunchKernelGGL(fs_k_replay_sample, dim3(batch), dim3(FS_REPLAY_THREADS), 0, (hipStream_t)stream, d_obs, d_masks,
                       d_labels, n_samples, d_table, channel_offset, channels, jitter ? 1 : 0, d_out_obs, d_out_mask,
                       d_out_label);
    return fs_hip_ok(hipGetLastError(), "fs_replay_sample launch") ? FS_OK : FS_ERR_HIP;
}
