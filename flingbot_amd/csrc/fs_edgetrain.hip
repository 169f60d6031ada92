// fs_edgetrain.hip -- what a SpatialValueNet train step needs besides the 16 -> 16 convolutions (fs_vntrain.hip) and the
// BatchNorm sites (fs_bntrain.hip): the first layer, the last layer at the one pixel per sample the loss reads, and Adam.
//   fs_convin_forward   y = conv3x3(x, W), x [B][C][64][64] with C in {1, 3, 4}, W [16][C][3][3], y [B][16][64][64]
//   fs_convin_wgrad     dW[oc][ic][ky][kx] = sum_{b,y,x} g[b,oc,y,x] x[b,ic,y+ky-1,x+kx-1]   (the observation needs no gradient)
//   fs_head_forward     pred[b] = the 16 -> 1 convolution of h at pixel pix[b]: 144 multiply-adds instead of 4096 x 144
//   fs_head_backward    dh = zeros with one clipped 3 x 3 x 16 patch gpred[b] W per image, dW = sum_b gpred[b] patch of h
//   fs_head_forward_pixels / fs_head_backward_pixels   the same layer at MANY pixels per image: a CSR list of labelled pixels
//   fs_adam_step        torch.optim.Adam's update of every parameter of an optimizer in one launch
// fp32, NCHW-contiguous, 64 x 64 maps, any batch >= 1: the conventions of fs_vntrain.hip / fs_bntrain.hip, with which this
// file shares no code.  Everything here is bound by memory or by launches, so it is plain VALU code: no MFMA.
//
// fs_k_convin_fwd<C>: a workgroup (4 wavefronts) owns an 8-row strip of one image.  The strip of x plus its one-row halo goes
//   into LDS (row stride 72 floats: image column x at x + 4, zero halo columns at 3 and 68), the weights too.  A thread owns
//   four neighbouring pixels of a row (wavefront w, lane l: row 4 (w & 1) + (l >> 4), columns 4 (l & 15) .. + 3) and eight
//   output channels (w >> 1); it holds the C x 3 x 6 patch in registers, reads each weight once (a broadcast) and stores
//   eight float4.  Every pixel's sum runs ic, ky, kx front to back: an image's bits do not depend on the batch it is in.
// fs_k_convin_wgrad<C>: a workgroup owns a 16-row strip.  Wavefront w owns output channels 4 w .. 4 w + 3, lane l the four
//   pixels of row (l >> 4) (mod 4) at columns 4 (l & 15) .. + 3, in four row groups one after the other; g comes straight from
//   global memory (each value is used once per wavefront), the x patch from LDS.  4 x 9 C accumulators per thread, added over
//   the lanes by a 6-step xor butterfly (every lane ends with the same bits), -> work[image * 4 + strip][16 C 9].
// fs_k_convin_wgrad_reduce: dW[e] = the 4 B partials in a fixed order: sixteen interleaved slices front to back, the sixteen
//   sums in a fixed tree.
// fs_k_head_fwd: one wavefront per sample; lane l takes terms l, l + 64, l + 128 of the 144, then the butterfly.
// fs_k_head_bwd: workgroup 0 sums dW over the batch front to back (thread e = one of the 144 weights; pixel and gpred of 256
//   samples at a time staged in LDS, so that the loads of h are independent of each other); workgroup 1 + (b, ic) writes one
//   plane of dh, four float4 per thread, every element either +0 or its patch value.
// fs_k_head_fwd_pixels: one wavefront per list entry (four to a workgroup); the entry's image is the last one whose offset is
//   <= the entry (a search over d_offsets, the same in every lane), the sum is fs_k_head_fwd's, term for term.
// fs_k_head_bwd_pixels_dh: a workgroup owns an 8-row strip of one image.  It zero-fills an LDS plane of the strip and its one-row
//   halo (the first layer's layout: row stride 72), drops gpred[l] at every listed pixel of the image that lies in it (distinct
//   pixels: no collisions), and after a barrier every thread forms four neighbouring pixels of eight channels as the nine-tap
//   sum over that plane, ky then kx ascending, and stores eight float4.  The cost does not depend on the list's length,
//   nothing is scattered into global memory, and an image's bits depend on its own list only.
// fs_k_head_bwd_pixels_dw: workgroup c owns list entries [64 c, 64 c + 64): image, pixel and gpred of each go into LDS, then
//   thread e (one of the 144 weights) adds them front to back -> work[c][144].  fs_k_convin_wgrad_reduce adds the chunks.
// fs_k_adam: blockIdx.y = segment, blockIdx.x strides over its elements.  The segment table is a kernel argument.
// No atomics and no arrival counters anywhere: every sum has a fixed order, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define ET_W 64           // map width and height
#define ET_PLANE 4096
#define ET_RS 72          // LDS row stride (floats)
#define ET_FROWS 8        // forward: rows per strip
#define ET_GROWS 16       // weight gradient: rows per strip
#define ET_GSTRIPS 4
#define ET_THREADS 256
#define ET_SLICES 16      // weight-gradient reduce: interleaved slices of the partials

// rows y0 - 1 .. y0 + ROWS of the C channels of image b -> LDS planes of (ROWS + 2) rows, zero outside the image and in the
// halo columns 3 and 68
template <int C, int ROWS>
__device__ __forceinline__ void et_stage_x(const float *__restrict__ x, int b, int y0, int t, float *s) {
    const float *src = x + (size_t)b * C * ET_PLANE;
    constexpr int NQ = C * (ROWS + 2) * 16;
    for (int idx = t; idx < NQ; idx += ET_THREADS) {
        const int ch = idx / ((ROWS + 2) * 16), rem = idx % ((ROWS + 2) * 16), r = rem >> 4, q = rem & 15, y = y0 - 1 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)y < (unsigned)ET_W) v = *(const float4 *)(src + ((size_t)ch * ET_W + y) * ET_W + 4 * q);
        *(float4 *)(s + (ch * (ROWS + 2) + r) * ET_RS + 4 + 4 * q) = v;
    }
    for (int idx = t; idx < C * (ROWS + 2) * 2; idx += ET_THREADS) s[(idx >> 1) * ET_RS + ((idx & 1) ? 68 : 3)] = 0.f;
}

// the 3 x 6 window of one channel around four pixels: p points at the first pixel's LDS slot in the row above
__device__ __forceinline__ void et_patch(const float *p, float (*xs)[6]) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const float *r = p + ky * ET_RS;
        const float4 m = *(const float4 *)r;
        xs[ky][0] = r[-1];
        xs[ky][1] = m.x; xs[ky][2] = m.y; xs[ky][3] = m.z; xs[ky][4] = m.w;
        xs[ky][5] = r[4];
    }
}

// ---- first layer, forward ----------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(ET_THREADS) void fs_k_convin_fwd(const float *__restrict__ x, const float *__restrict__ W, int batch,
                                                              float *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) float s_x[C * (ET_FROWS + 2) * ET_RS];
    __shared__ float s_w[16 * C * 9];
    const int t = threadIdx.x, b = blockIdx.x >> 3, strip = blockIdx.x & 7, y0 = strip * ET_FROWS;
    if (b >= batch) return;
    et_stage_x<C, ET_FROWS>(x, b, y0, t, s_x);
    for (int i = t; i < 16 * C * 9; i += ET_THREADS) s_w[i] = W[i];
    __syncthreads();
    const int l = t & 63, wv = t >> 6, row = 4 * (wv & 1) + (l >> 4), q = l & 15, oc0 = 8 * (wv >> 1);
    float xs[C][3][6];
#pragma unroll
    for (int ic = 0; ic < C; ++ic) et_patch(s_x + (ic * (ET_FROWS + 2) + row) * ET_RS + 4 + 4 * q, xs[ic]);
    float *dst = y + (((size_t)b * 16 + oc0) * ET_W + y0 + row) * ET_W + 4 * q;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const float *w = s_w + (oc0 + o) * C * 9;   // the same address in every lane: a broadcast
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ic = 0; ic < C; ++ic)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float wt = w[(ic * 3 + ky) * 3 + kx];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = acc[j] + wt * xs[ic][ky][j + kx];
                }
        *(float4 *)(dst + (size_t)o * ET_PLANE) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// ---- first layer, weight gradient: per-strip partials ---------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(ET_THREADS) void fs_k_convin_wgrad(const float *__restrict__ x, const float *__restrict__ g, int batch,
                                                                float *__restrict__ work) {
    __shared__ __attribute__((aligned(16))) float s_x[C * (ET_GROWS + 2) * ET_RS];
    __shared__ float s_out[16 * C * 9];
    const int t = threadIdx.x, b = blockIdx.x >> 2, strip = blockIdx.x & 3, y0 = strip * ET_GROWS;
    if (b >= batch) return;
    const int l = t & 63, wv = t >> 6, rp = l >> 4, q = l & 15, oc0 = 4 * wv;
    et_stage_x<C, ET_GROWS>(x, b, y0, t, s_x);
    __syncthreads();
    float acc[4][C * 9];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int e = 0; e < C * 9; ++e) acc[o][e] = 0.f;
    const float *gsrc = g + (((size_t)b * 16 + oc0) * ET_W + y0 + rp) * ET_W + 4 * q;
#pragma unroll 1
    for (int it = 0; it < ET_GROWS / 4; ++it) {
        const int row = 4 * it + rp;
        float gv[4][4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float4 v = *(const float4 *)(gsrc + (size_t)o * ET_PLANE + (size_t)(4 * it) * ET_W);
            gv[o][0] = v.x; gv[o][1] = v.y; gv[o][2] = v.z; gv[o][3] = v.w;
        }
#pragma unroll
        for (int ic = 0; ic < C; ++ic) {
            float xs[3][6];
            et_patch(s_x + (ic * (ET_GROWS + 2) + row) * ET_RS + 4 + 4 * q, xs);
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[o][(ic * 3 + ky) * 3 + kx] = acc[o][(ic * 3 + ky) * 3 + kx] + gv[o][j] * xs[ky][j + kx];
        }
    }
    // the 64 lanes' sums by an xor butterfly: each step adds the same two numbers in both lanes, all lanes end with the same bits
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int e = 0; e < C * 9; ++e) {
            float v = acc[o][e];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
            if (l == 0) s_out[(oc0 + o) * C * 9 + e] = v;
        }
    __syncthreads();
    float *dst = work + (size_t)blockIdx.x * (16 * C * 9);
    for (int e = t; e < 16 * C * 9; e += ET_THREADS) dst[e] = s_out[e];
}

// 512 threads = 32 elements x 16 slices; slice s adds partials s, s + 16, ... (there are 4 * batch) front to back
__global__ __launch_bounds__(512) void fs_k_convin_wgrad_reduce(const float *__restrict__ work, int n_partials, int n_elements,
                                                                float *__restrict__ dw) {
    __shared__ float s[ET_SLICES][32];
    const int t = threadIdx.x, el = t & 31, sl = t >> 5, e = blockIdx.x * 32 + el;
    float sum = 0.f;
    if (e < n_elements) {
#pragma unroll 8   // eight loads in flight; the additions keep their order
        for (int p = sl; p < n_partials; p += ET_SLICES) sum = sum + work[(size_t)p * n_elements + e];
    }
    s[sl][el] = sum;
    __syncthreads();
    if (sl == 0 && e < n_elements) {
        float v[ET_SLICES];
#pragma unroll
        for (int i = 0; i < ET_SLICES; ++i) v[i] = s[i][el];
#pragma unroll
        for (int w = 1; w < ET_SLICES; w *= 2)
#pragma unroll
            for (int i = 0; i < ET_SLICES; i += 2 * w) v[i] = v[i] + v[i + w];
        dw[e] = v[0];
    }
}

// ---- last layer at one pixel per sample ------------------------------------------------------------------------------------
__device__ __forceinline__ int et_pixel(const int *__restrict__ pix, int b) {
    const int p = pix[b];
    return p < 0 ? 0 : (p > ET_PLANE - 1 ? ET_PLANE - 1 : p);   // a bad index must not become a bad address
}

// term e = ic * 9 + ky * 3 + kx of the sample at (py, px): the value of h under that tap, 0 outside the image
__device__ __forceinline__ float et_tap(const float *__restrict__ hb, int e, int py, int px) {
    const int ic = e / 9, tap = e % 9, yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
    if ((unsigned)yy >= (unsigned)ET_W || (unsigned)xx >= (unsigned)ET_W) return 0.f;
    return hb[(size_t)ic * ET_PLANE + yy * ET_W + xx];
}

__global__ __launch_bounds__(64) void fs_k_head_fwd(const float *__restrict__ h, const float *__restrict__ W,
                                                    const int *__restrict__ pix, float *__restrict__ pred) {
    const int b = blockIdx.x, l = threadIdx.x, p = et_pixel(pix, b), py = p >> 6, px = p & 63;
    const float *hb = h + (size_t)b * 16 * ET_PLANE;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = l + 64 * k;
        if (e < 144) v = v + W[e] * et_tap(hb, e, py, px);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    if (l == 0) pred[b] = v;
}

__global__ __launch_bounds__(ET_THREADS) void fs_k_head_bwd(const float *__restrict__ h, const float *__restrict__ W,
                                                            const int *__restrict__ pix, const float *__restrict__ gpred, int batch,
                                                            float *__restrict__ dh, float *__restrict__ dw) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {   // dW, front to back over the batch
        __shared__ int s_pix[ET_THREADS];
        __shared__ float s_g[ET_THREADS];
        float sum = 0.f;
        for (int b0 = 0; b0 < batch; b0 += ET_THREADS) {
            const int n = batch - b0 < ET_THREADS ? batch - b0 : ET_THREADS;
            __syncthreads();
            if (t < n) { s_pix[t] = et_pixel(pix, b0 + t); s_g[t] = gpred[b0 + t]; }
            __syncthreads();
            if (t < 144) {
#pragma unroll 8   // eight loads in flight; the additions keep their order
                for (int i = 0; i < n; ++i) {
                    const int p = s_pix[i];
                    sum = sum + s_g[i] * et_tap(h + (size_t)(b0 + i) * 16 * ET_PLANE, t, p >> 6, p & 63);
                }
            }
        }
        if (t < 144) dw[t] = sum;
        return;
    }
    const int plane = blockIdx.x - 1, b = plane >> 4, ic = plane & 15;
    const int p = et_pixel(pix, b), py = p >> 6, px = p & 63;
    const float gp = gpred[b];
    float wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = gp * W[ic * 9 + k];
    float4 *dst = (float4 *)(dh + (size_t)plane * ET_PLANE);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int f = t + ET_THREADS * k, yy = f >> 4, x0 = 4 * (f & 15), ky = yy - py + 1;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)ky < 3u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kx = x0 + j - px + 1;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (kx == c) o[j] = ky == 0 ? wt[c] : (ky == 1 ? wt[3 + c] : wt[6 + c]);
            }
        }
        dst[f] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- last layer at a list of pixels per image -------------------------------------------------------------------------------
#define ET_PCHUNK 64      // list entries per weight-gradient partial

__device__ __forceinline__ int et_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the image that owns list entry l: the last b in [0, batch) with offsets[b] <= l (images without entries are passed over).
// Reads offsets[1 .. batch - 1] only and returns a valid image whatever the table holds.
__device__ __forceinline__ int et_image_of(const int *__restrict__ offsets, int batch, int l) {
    int lo = 0, hi = batch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= l) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ET_THREADS) void fs_k_head_fwd_pixels(const float *__restrict__ h, const float *__restrict__ W,
                                                                   const int *__restrict__ offsets, const int *__restrict__ pix,
                                                                   int batch, int n_pixels, float *__restrict__ pred) {
    const int l = threadIdx.x & 63, entry = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (entry >= n_pixels) return;   // (a whole wavefront)
    const int b = et_image_of(offsets, batch, entry), p = et_pixel(pix, entry), py = p >> 6, px = p & 63;
    const float *hb = h + (size_t)b * 16 * ET_PLANE;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = l + 64 * k;
        if (e < 144) v = v + W[e] * et_tap(hb, e, py, px);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    if (l == 0) pred[entry] = v;
}

__global__ __launch_bounds__(ET_THREADS) void fs_k_head_bwd_pixels_dh(const float *__restrict__ W, const int *__restrict__ offsets,
                                                                      const int *__restrict__ pix, const float *__restrict__ gpred,
                                                                      int batch, int n_pixels, float *__restrict__ dh) {
    __shared__ __attribute__((aligned(16))) float s_g[(ET_FROWS + 2) * ET_RS];
    __shared__ float s_w[144];
    const int t = threadIdx.x, b = blockIdx.x >> 3, strip = blockIdx.x & 7, y0 = strip * ET_FROWS;
    if (b >= batch) return;
    for (int i = t; i < (ET_FROWS + 2) * ET_RS; i += ET_THREADS) s_g[i] = 0.f;
    if (t < 144) s_w[t] = W[t];
    __syncthreads();
    const int begin = et_clamp(offsets[b], 0, n_pixels), end = et_clamp(offsets[b + 1], begin, n_pixels);
    for (int i = begin + t; i < end; i += ET_THREADS) {
        const int p = et_pixel(pix, i), r = (p >> 6) - y0 + 1;   // LDS row of the pixel: 0 .. ET_FROWS + 1 inside strip and halo
        if ((unsigned)r < (unsigned)(ET_FROWS + 2)) s_g[r * ET_RS + 4 + (p & 63)] = gpred[i];
    }
    __syncthreads();
    const int l = t & 63, wv = t >> 6, row = 4 * (wv & 1) + (l >> 4), q = l & 15, ic0 = 8 * (wv >> 1);
    float gs[3][6];   // gs[r][c] = the gradient plane at (y0 + row - 1 + r, 4 q - 1 + c)
    et_patch(s_g + row * ET_RS + 4 + 4 * q, gs);
    float *dst = dh + (((size_t)b * 16 + ic0) * ET_W + y0 + row) * ET_W + 4 * q;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const float *w = s_w + (ic0 + o) * 9;   // the same address in every lane: a broadcast
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        // tap (ky, kx) of the pixel at (y - ky + 1, x - kx + 1) lies on (y, x)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float wt = w[ky * 3 + kx];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = acc[j] + gs[2 - ky][j + 2 - kx] * wt;
            }
        *(float4 *)(dst + (size_t)o * ET_PLANE) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

__global__ __launch_bounds__(ET_THREADS) void fs_k_head_bwd_pixels_dw(const float *__restrict__ h, const int *__restrict__ offsets,
                                                                      const int *__restrict__ pix, const float *__restrict__ gpred,
                                                                      int batch, int n_pixels, float *__restrict__ work) {
    __shared__ int s_img[ET_PCHUNK];
    __shared__ int s_pix[ET_PCHUNK];
    __shared__ float s_gp[ET_PCHUNK];
    const int t = threadIdx.x, first = blockIdx.x * ET_PCHUNK;
    const int n = n_pixels - first < ET_PCHUNK ? n_pixels - first : ET_PCHUNK;
    if (t < n) {
        s_img[t] = et_image_of(offsets, batch, first + t);
        s_pix[t] = et_pixel(pix, first + t);
        s_gp[t] = gpred[first + t];
    }
    __syncthreads();
    if (t >= 144) return;
    float sum = 0.f;
#pragma unroll 8   // eight loads in flight; the additions keep their order
    for (int i = 0; i < n; ++i) {
        const int p = s_pix[i];
        sum = sum + s_gp[i] * et_tap(h + (size_t)s_img[i] * 16 * ET_PLANE, t, p >> 6, p & 63);
    }
    work[(size_t)blockIdx.x * 144 + t] = sum;
}

// ---- Adam ------------------------------------------------------------------------------------------------------------------
#define ET_ADAM_SEGMENTS 80   // per launch: 80 * 40 bytes of kernel argument

struct et_adam_table {
    fs_adam_segment seg[ET_ADAM_SEGMENTS];
};

// torch.optim.Adam (single-tensor form) in fp32: g' = g + wd p; m += (g' - m)(1 - b1); v = b2 v + (1 - b2) g' g';
// p -= step_size * m / (sqrt(v) / bc2_sqrt + eps), step_size = lr / bc1
__global__ __launch_bounds__(ET_THREADS) void fs_k_adam(const et_adam_table table, float one_minus_beta1, float beta2,
                                                        float one_minus_beta2, float eps, float weight_decay, float step_size,
                                                        float bc2_sqrt) {
    const fs_adam_segment sg = table.seg[blockIdx.y];
    float *__restrict__ p = (float *)sg.param;
    const float *__restrict__ g = (const float *)sg.grad;
    float *__restrict__ m = (float *)sg.exp_avg;
    float *__restrict__ v = (float *)sg.exp_avg_sq;
    for (long long i = (long long)blockIdx.x * ET_THREADS + threadIdx.x; i < sg.count; i += (long long)gridDim.x * ET_THREADS) {
        const float pi = p[i];
        float gi = g[i];
        if (weight_decay != 0.f) gi = gi + weight_decay * pi;
        const float mi = m[i] + (gi - m[i]) * one_minus_beta1;
        const float vi = v[i] * beta2 + (one_minus_beta2 * gi) * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------
static bool et_channels_served(int channels) { return channels == 1 || channels == 3 || channels == 4; }

extern "C" {

size_t fs_convin_work_bytes(int channels, int batch, int dim) {
    if (!et_channels_served(channels) || batch < 1 || dim != ET_W) return 0;
    return (size_t)batch * ET_GSTRIPS * 16 * channels * 9 * sizeof(float);
}

int fs_convin_forward(const float *d_x, const float *d_w, int channels, int batch, int dim, float *d_y, void *stream) {
    if (!d_x || !d_w || !d_y || !et_channels_served(channels) || batch < 1 || dim != ET_W) {
        fs_set_error("fs_convin_forward: bad arguments (the kernels are built for [batch >= 1][1, 3 or 4][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_w, d_y})) {   // moved as float4
        fs_set_error("fs_convin_forward: d_x, d_w and d_y must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)batch * 8), block(ET_THREADS);
    if (channels == 1) hipLaunchKernelGGL(fs_k_convin_fwd<1>, grid, block, 0, st, d_x, d_w, batch, d_y);
    else if (channels == 3) hipLaunchKernelGGL(fs_k_convin_fwd<3>, grid, block, 0, st, d_x, d_w, batch, d_y);
    else hipLaunchKernelGGL(fs_k_convin_fwd<4>, grid, block, 0, st, d_x, d_w, batch, d_y);
    return fs_hip_ok(hipGetLastError(), "fs_convin_forward launch") ? FS_OK : FS_ERR_HIP;
}

int fs_convin_wgrad(const float *d_x, const float *d_g, int channels, int batch, int dim, float *d_dw, void *d_work, void *stream) {
    if (!d_x || !d_g || !d_dw || !d_work || !et_channels_served(channels) || batch < 1 || dim != ET_W) {
        fs_set_error("fs_convin_wgrad: bad arguments (the kernels are built for [batch >= 1][1, 3 or 4][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_g, d_dw, d_work})) {
        fs_set_error("fs_convin_wgrad: d_x, d_g, d_dw and d_work must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)batch * ET_GSTRIPS), block(ET_THREADS);
    float *work = (float *)d_work;
    if (channels == 1) hipLaunchKernelGGL(fs_k_convin_wgrad<1>, grid, block, 0, st, d_x, d_g, batch, work);
    else if (channels == 3) hipLaunchKernelGGL(fs_k_convin_wgrad<3>, grid, block, 0, st, d_x, d_g, batch, work);
    else hipLaunchKernelGGL(fs_k_convin_wgrad<4>, grid, block, 0, st, d_x, d_g, batch, work);
    const int n_elements = 16 * channels * 9;
    hipLaunchKernelGGL(fs_k_convin_wgrad_reduce, dim3((n_elements + 31) / 32), dim3(512), 0, st, (const float *)work,
                       batch * ET_GSTRIPS, n_elements, d_dw);
    return fs_hip_ok(hipGetLastError(), "fs_convin_wgrad launch") ? FS_OK : FS_ERR_HIP;
}

int fs_head_forward(const float *d_h, const float *d_w, const int *d_pix, int batch, int dim, float *d_pred, void *stream) {
    if (!d_h || !d_w || !d_pix || !d_pred || batch < 1 || dim != ET_W) {
        fs_set_error("fs_head_forward: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_h, d_w, d_pix, d_pred})) {
        fs_set_error("fs_head_forward: d_h, d_w, d_pix and d_pred must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    hipLaunchKernelGGL(fs_k_head_fwd, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, d_h, d_w, d_pix, d_pred);
    return fs_hip_ok(hipGetLastError(), "fs_head_forward launch") ? FS_OK : FS_ERR_HIP;
}

int fs_head_backward(const float *d_h, const float *d_w, const int *d_pix, const float *d_gpred, int batch, int dim, float *d_dh,
                     float *d_dw, void *stream) {
    if (!d_h || !d_w || !d_pix || !d_gpred || !d_dh || !d_dw || batch < 1 || dim != ET_W) {
        fs_set_error("fs_head_backward: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_h, d_w, d_pix, d_gpred, d_dh, d_dw})) {
        fs_set_error("fs_head_backward: every pointer must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    if (d_dh == d_h) {
        fs_set_error("fs_head_backward: in place is not supported (d_dh == d_h)");
        return FS_ERR_ARG;
    }
    hipLaunchKernelGGL(fs_k_head_bwd, dim3((unsigned)batch * 16 + 1), dim3(ET_THREADS), 0, (hipStream_t)stream, d_h, d_w, d_pix,
                       d_gpred, batch, d_dh, d_dw);
    return fs_hip_ok(hipGetLastError(), "fs_head_backward launch") ? FS_OK : FS_ERR_HIP;
}

size_t fs_head_pixels_work_bytes(int batch, int n_pixels, int dim) {
    if (batch < 1 || n_pixels < 1 || dim != ET_W) return 0;
    return (((size_t)n_pixels + ET_PCHUNK - 1) / ET_PCHUNK) * 144 * sizeof(float);
}

int fs_head_forward_pixels(const float *d_h, const float *d_w, const int *d_offsets, const int *d_pix, int batch, int n_pixels,
                           int dim, float *d_pred, void *stream) {
    if (!d_h || !d_w || !d_offsets || !d_pix || !d_pred || batch < 1 || n_pixels < 1 || dim != ET_W) {
        fs_set_error("fs_head_forward_pixels: bad arguments (the kernels are built for [batch >= 1][16][64][64] and n_pixels >= 1)");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_h, d_w, d_offsets, d_pix, d_pred})) {
        fs_set_error("fs_head_forward_pixels: every pointer must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    hipLaunchKernelGGL(fs_k_head_fwd_pixels, dim3(((unsigned)n_pixels + 3) / 4), dim3(ET_THREADS), 0, (hipStream_t)stream, d_h, d_w,
                       d_offsets, d_pix, batch, n_pixels, d_pred);
    return fs_hip_ok(hipGetLastError(), "fs_head_forward_pixels launch") ? FS_OK : FS_ERR_HIP;
}

int fs_head_backward_pixels(const float *d_h, const float *d_w, const int *d_offsets, const int *d_pix, const float *d_gpred,
                            int batch, int n_pixels, int dim, float *d_dh, float *d_dw, void *d_work, void *stream) {
    if (!d_h || !d_w || !d_offsets || !d_pix || !d_gpred || !d_dh || !d_dw || !d_work || batch < 1 || n_pixels < 1 || dim != ET_W) {
        fs_set_error("fs_head_backward_pixels: bad arguments (the kernels are built for [batch >= 1][16][64][64] and n_pixels >= 1)");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_h, d_w, d_offsets, d_pix, d_gpred, d_dh, d_dw, d_work})) {
        fs_set_error("fs_head_backward_pixels: every pointer must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    if (d_dh == d_h) {
        fs_set_error("fs_head_backward_pixels: in place is not supported (d_dh == d_h)");
        return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    float *work = (float *)d_work;
    const int n_chunks = (n_pixels + ET_PCHUNK - 1) / ET_PCHUNK;
    hipLaunchKernelGGL(fs_k_head_bwd_pixels_dh, dim3((unsigned)batch * 8), dim3(ET_THREADS), 0, st, d_w, d_offsets, d_pix, d_gpred,
                       batch, n_pixels, d_dh);
    hipLaunchKernelGGL(fs_k_head_bwd_pixels_dw, dim3((unsigned)n_chunks), dim3(ET_THREADS), 0, st, d_h, d_offsets, d_pix, d_gpred,
                       batch, n_pixels, work);
    hipLaunchKernelGGL(fs_k_convin_wgrad_reduce, dim3((144 + 31) / 32), dim3(512), 0, st, (const float *)work, n_chunks, 144, d_dw);
    return fs_hip_ok(hipGetLastError(), "fs_head_backward_pixels launch") ? FS_OK : FS_ERR_HIP;
}

int fs_adam_step(const fs_adam_segment *segments, int n_segments, double lr, double beta1, double beta2, double eps,
                 double weight_decay, double bias_correction1, double bias_correction2, void *stream) {
    if (!segments || n_segments < 1 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
        !(weight_decay >= 0.0) || !(bias_correction1 > 0.0 && bias_correction1 <= 1.0) || !(bias_correction2 > 0.0 && bias_correction2 <= 1.0)) {
        fs_set_error("fs_adam_step: bad arguments (a segment table, lr, eps, weight_decay >= 0, betas in [0, 1), bias corrections in (0, 1])");
        return FS_ERR_ARG;
    }
    for (int i = 0; i < n_segments; ++i) {
        const fs_adam_segment &s = segments[i];
        if (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq || s.count < 1 ||
            (((uintptr_t)s.param | (uintptr_t)s.grad | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq) & 3)) {
            fs_set_error("fs_adam_step: every segment has four non-null float pointers and count >= 1");
            return FS_ERR_ARG;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const float step_size = (float)(lr / bias_correction1), bc2_sqrt = (float)std::sqrt(bias_correction2);
    for (int first = 0; first < n_segments; first += ET_ADAM_SEGMENTS) {
        const int n = n_segments - first < ET_ADAM_SEGMENTS ? n_segments - first : ET_ADAM_SEGMENTS;
        et_adam_table table;
        long long most = 0;
        for (int i = 0; i < n; ++i) {
            table.seg[i] = segments[first + i];
            if (table.seg[i].count > most) most = table.seg[i].count;
        }
        for (int i = n; i < ET_ADAM_SEGMENTS; ++i) table.seg[i] = fs_adam_segment{nullptr, nullptr, nullptr, nullptr, 0};
        long long bx = (most + ET_THREADS - 1) / ET_THREADS;
        if (bx > 64) bx = 64;   // longer segments stride
        hipLaunchKernelGGL(fs_k_adam, dim3((unsigned)bx, (unsigned)n), dim3(ET_THREADS), 0, st, table, (float)(1.0 - beta1), (float)beta2,
                           (float)(1.0 - beta2), (float)eps, (float)weight_decay, step_size, bc2_sqrt);
    }
    return fs_hip_ok(hipGetLastError(), "fs_adam_step launch") ? FS_OK : FS_ERR_HIP;
}

}  // extern "C"
