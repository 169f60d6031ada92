// fs_panels.hip -- the picture of a chosen action (flingbot_amd/report.py): value range and the five-panel strip; at the end of
// the file the strip of a look-ahead step (fs_lane_panels) and that of a probed map (fs_probe_panels).
//
// Reference: environment/utils.py visualize_action (:369-432) builds a matplotlib figure on the host for every chosen action
// (simEnv.py:653-654): the value map under `jet` with vmin / vmax over all maps of the primitive (:396-398), the transformed
// RGB with draw_action's cv2 overlay at thickness 1 (:403-409) and the pre-transform image with the overlay at thickness 3
// (:414-422), each overlay shown with alpha 0.9.  Its inputs are on the device at that moment, so here the strips of all ready
// episodes are composed in ONE launch:  before | value map | transformed RGB + action | before + action | after.
//
// Every rule is integer or single-rounded fp32 (include/flingsim.h has them in full; tests/report_reference.py restates them
// in numpy and the kernels are compared with it byte for byte):
//   float -> uint8   trunc(clamp(x * 255, 0, 255)) in fp32 (replay.quantize)
//   sampling         nearest: source index = (dst * src_size) / panel, integer division, per axis; overlays are drawn at the
//                    source's resolution and sampled with it
//   value colour     t = (v - vmin) / (vmax - vmin), one fp32 subtraction each and the correctly rounded fp32 quotient, formed as
//                    (float)((double)a / (double)b): a double quotient rounded to float IS the correctly rounded float quotient
//                    (53 >= 2 * 24 + 2 bits), whatever the compiler's fp32 division expands to;  index = clamp((int)(t * 256), 0,
//                    255), 0 for vmax == vmin or a non-finite v;  colour = jet[index] (fs_jet_table.h)
//   ring             (2R - t)^2 <= 4 d^2 <= (2R + t)^2, d^2 the squared integer distance to the centre
//   segment          a -> b, v = b - a, w = p - a, L = v.v:  w.v <= 0: 4 |w|^2 <= t^2;  w.v >= L: 4 |p - b|^2 <= t^2;
//                    else 4 (w x v)^2 <= t^2 L;  all in int64 (|coordinate| <= 8191, t <= 64, pixel < 4096: below 2^60)
//   blend            the LAST primitive that covers the pixel:  (9 * colour + base + 5) / 10 per channel, integer division
//
// fs_k_action_panels: grid (groups of 1024 pixels, actions), 256 threads, 4 consecutive pixels = 12 bytes = 3 dwords per thread.
// The action's record and the jet table sit in LDS.  Every output pixel is a function of its own record alone, so a strip does
// not depend on the batch it is composed in.  15 panel^2 bytes are written per action and the reads are served by L2 (the
// sources are at most 3 S^2 + 5 D^2 floats), but the overlay tests (int64) and the value panel's double division keep it
// well below the write bandwidth (EXPERIMENTS R16.1); the download that follows costs forty times the launch.
// fs_k_value_range: one workgroup per item, so the result depends on neither B nor the item's place; the item table travels as
// a kernel argument (no copy, no host synchronisation).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/flingsim.h"
#include "fs_context.h"
#include "fs_jet_table.h"

static_assert(sizeof(fs_panel_record) == 624, "flingbot_amd/report.py PANEL_RECORD mirrors this layout");
static_assert(sizeof(fs_range_item) == 16, "flingbot_amd/report.py RANGE_ITEM mirrors this layout");

#define FS_PANEL_THREADS 256
#define FS_PANEL_PIXELS_PER_THREAD 4
#define FS_PANEL_LIMIT 4096
#define FS_PANEL_COORD_LIMIT 8191
#define FS_PANEL_THICKNESS_LIMIT 64
#define FS_RANGE_THREADS 256
#define FS_RANGE_CHUNK 128  // items per launch: 2 KiB of kernel arguments

static const unsigned char fs_jet_host[FS_JET_ENTRIES * 3] = {FS_JET_VALUES};
__constant__ unsigned char fs_jet_device[FS_JET_ENTRIES * 3] = {FS_JET_VALUES};

extern "C" int fs_jet_table(unsigned char *out, int n_bytes) {
    if (!out || n_bytes != FS_JET_ENTRIES * 3) {
        fs_set_error("fs_jet_table: out must hold 768 bytes");
        return FS_ERR_ARG;
    }
    memcpy(out, fs_jet_host, sizeof(fs_jet_host));
    return FS_OK;
}

// ---- value range ----------------------------------------------------------------------------------------------------------
struct FsRangeArgs {
    fs_range_item item[FS_RANGE_CHUNK];
};

__device__ __forceinline__ void fs_range_take(float x, float &lo, float &hi) {
    if (__builtin_isfinite(x)) {
        lo = fminf(lo, x);
        hi = fmaxf(hi, x);
    }
}

__global__ __launch_bounds__(FS_RANGE_THREADS) void fs_k_value_range(FsRangeArgs args, float *__restrict__ out) {
    __shared__ float wave_lo[FS_RANGE_THREADS / 64], wave_hi[FS_RANGE_THREADS / 64];
    const int tid = threadIdx.x;
    const float *__restrict__ src = args.item[blockIdx.x].values;
    const long long count = args.item[blockIdx.x].count;
    float lo = INFINITY, hi = -INFINITY;
    // the 16-byte aligned middle in float4s, the (up to 3) floats in front of it and the tail one by one
    long long head = (long long)(((16 - ((uintptr_t)src & 15)) & 15) / 4);
    if (head > count) head = count;
    const long long quads = (count - head) / 4;
    const float4 *__restrict__ mid = reinterpret_cast<const float4 *>(src + head);
    for (long long q = tid; q < quads; q += FS_RANGE_THREADS) {
        const float4 v = mid[q];
        fs_range_take(v.x, lo, hi);
        fs_range_take(v.y, lo, hi);
        fs_range_take(v.z, lo, hi);
        fs_range_take(v.w, lo, hi);
    }
    if (tid < head) fs_range_take(src[tid], lo, hi);
    const long long tail = head + 4 * quads;
    if (tail + tid < count) fs_range_take(src[tail + tid], lo, hi);   // (fewer than 4 floats are left)
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
    }
    if ((tid & 63) == 0) {
        wave_lo[tid >> 6] = lo;
        wave_hi[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < FS_RANGE_THREADS / 64; ++w) {
            lo = fminf(lo, wave_lo[w]);
            hi = fmaxf(hi, wave_hi[w]);
        }
        const bool any = lo <= hi;   // (+inf, -inf) when no value was finite
        // x + 0.0f: a minimum or maximum of -0.0 and +0.0 is reported as +0.0, whichever the reduction met first
        out[2 * blockIdx.x] = any ? lo + 0.0f : 0.0f;
        out[2 * blockIdx.x + 1] = any ? hi + 0.0f : 0.0f;
    }
}

extern "C" int fs_value_range(const fs_range_item *items, int n_items, float *d_out, void *stream) {
    if (!items || !d_out || n_items < 1) {
        fs_set_error("fs_value_range: a null table or output, or fewer than one item");
        return FS_ERR_ARG;
    }
    for (int k = 0; k < n_items; ++k) {
        if (!items[k].values || items[k].count < 1 || ((uintptr_t)items[k].values & 3)) {
            fs_set_error("fs_value_range: item " + std::to_string(k) + " has a null or misaligned pointer or a count below 1");
            return FS_ERR_ARG;
        }
    }
    for (int first = 0; first < n_items; first += FS_RANGE_CHUNK) {
        const int n = n_items - first < FS_RANGE_CHUNK ? n_items - first : FS_RANGE_CHUNK;
        FsRangeArgs args;
        memset(&args, 0, sizeof(args));
        memcpy(args.item, items + first, sizeof(fs_range_item) * (size_t)n);
        hipLaunchKernelGGL(fs_k_value_range, dim3(n), dim3(FS_RANGE_THREADS), 0, (hipStream_t)stream, args, d_out + 2 * (size_t)first);
    }
    return fs_hip_ok(hipGetLastError(), "fs_value_range launch") ? FS_OK : FS_ERR_HIP;
}

// ---- action strips ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fs_quantize(float x) { return (int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

// prim: kind, y0, x0, y1, x1, t, r, g, b
__device__ __forceinline__ bool fs_prim_covers(const int *prim, int py, int px) {
    const long long t = prim[5];
    if (prim[0] == FS_PANEL_RING) {
        const long long dy = py - prim[1], dx = px - prim[2], r2 = 2 * (long long)prim[3];
        const long long d4 = 4 * (dy * dy + dx * dx), inner = r2 - t, outer = r2 + t;
        return inner * inner <= d4 && d4 <= outer * outer;
    }
    const long long vy = prim[3] - prim[1], vx = prim[4] - prim[2], wy = py - prim[1], wx = px - prim[2];
    const long long len = vy * vy + vx * vx, along = wy * vy + wx * vx;
    if (along <= 0) return 4 * (wy * wy + wx * wx) <= t * t;
    if (along >= len) {
        const long long ey = py - prim[3], ex = px - prim[4];
        return 4 * (ey * ey + ex * ex) <= t * t;
    }
    const long long cross = wy * vx - wx * vy;
    return 4 * cross * cross <= t * t * len;
}

// one source pixel's colour under the overlay list: the last primitive that covers it, blended once
__device__ __forceinline__ uint32_t fs_overlay(const int *prims, int n, int py, int px, int r, int g, int b) {
    int hit = -1;
    for (int k = 0; k < n; ++k)
        if (fs_prim_covers(prims + 9 * k, py, px)) hit = k;
    if (hit >= 0) {
        const int *c = prims + 9 * hit + 6;
        r = (9 * c[0] + r + 5) / 10;
        g = (9 * c[1] + g + 5) / 10;
        b = (9 * c[2] + b + 5) / 10;
    }
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

__device__ __forceinline__ uint32_t fs_rgb_at(const float *__restrict__ planes, int size, int sy, int sx) {
    const size_t plane = (size_t)size * size, at = (size_t)sy * size + sx;
    return (uint32_t)fs_quantize(planes[at]) | ((uint32_t)fs_quantize(planes[plane + at]) << 8) |
           ((uint32_t)fs_quantize(planes[2 * plane + at]) << 16);
}

// the value-colour rule: v under jet over (vmin, vmax)
__device__ __forceinline__ uint32_t fs_value_colour(const unsigned char *jet, float v, float vmin, float vmax) {
    int index = 0;
    if (vmax != vmin && __builtin_isfinite(v)) {
        const float t = (float)((double)(v - vmin) / (double)(vmax - vmin));
        const float f = t * 256.0f;
        index = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);   // clamp((int)f, 0, 255); 0 for a NaN
    }
    return (uint32_t)jet[3 * index] | ((uint32_t)jet[3 * index + 1] << 8) | ((uint32_t)jet[3 * index + 2] << 16);
}

// pixel (y, x5) of the strip, x5 in [0, 5 panel): R | G << 8 | B << 16
__device__ __forceinline__ uint32_t fs_strip_pixel(const fs_panel_record &rec, const unsigned char *jet, int D, int S, int panel,
                                                   int y, int x5) {
    const int which = x5 / panel, x = x5 - which * panel;
    if (which == 1) {  // the value map under jet
        const int sy = (y * D) / panel, sx = (x * D) / panel;
        return fs_value_colour(jet, rec.value_map[(size_t)sy * D + sx], rec.range[0], rec.range[1]);
    }
    if (which == 2) {  // what the net saw, with the action at thickness 1
        const int sy = (y * D) / panel, sx = (x * D) / panel;
        const uint32_t base = fs_rgb_at(rec.stack, D, sy, sx);
        return fs_overlay(&rec.small[0][0], rec.n_small, sy, sx, base & 255, (base >> 8) & 255, (base >> 16) & 255);
    }
    const int sy = (y * S) / panel, sx = (x * S) / panel;
    if (which == 4) return rec.after ? fs_rgb_at(rec.after, S, sy, sx) : 0u;
    const uint32_t base = fs_rgb_at(rec.before, S, sy, sx);
    if (which == 0) return base;
    return fs_overlay(&rec.large[0][0], rec.n_large, sy, sx, base & 255, (base >> 8) & 255, (base >> 16) & 255);
}

// the first `valid` of a thread's four consecutive pixels (R | G << 8 | B << 16 each) to dst
__device__ __forceinline__ void fs_store_pixels(unsigned char *dst, const uint32_t (&px)[FS_PANEL_PIXELS_PER_THREAD], int valid) {
    if (valid == FS_PANEL_PIXELS_PER_THREAD && ((uintptr_t)dst & 3) == 0) {  // RGB RGB RGB RGB as three dwords
        uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
        d32[0] = px[0] | (px[1] << 24);
        d32[1] = (px[1] >> 8) | (px[2] << 16);
        d32[2] = (px[2] >> 16) | (px[3] << 8);
    } else {  // an odd panel puts every other strip off the dword grid; the last pixels of a strip
        for (int j = 0; j < valid; ++j) {
            dst[3 * j] = (unsigned char)(px[j] & 255);
            dst[3 * j + 1] = (unsigned char)((px[j] >> 8) & 255);
            dst[3 * j + 2] = (unsigned char)((px[j] >> 16) & 255);
        }
    }
}

__global__ __launch_bounds__(FS_PANEL_THREADS) void fs_k_action_panels(const fs_panel_record *__restrict__ table, int D, int S,
                                                                       int panel, unsigned char *__restrict__ out) {
    __shared__ fs_panel_record rec;
    __shared__ unsigned char jet[FS_JET_ENTRIES * 3];
    const int tid = threadIdx.x, b = blockIdx.y;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(table + b);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&rec);
        for (int q = tid; q < (int)(sizeof(fs_panel_record) / 4); q += FS_PANEL_THREADS) dst[q] = src[q];
        const uint32_t *jsrc = reinterpret_cast<const uint32_t *>(fs_jet_device);
        uint32_t *jdst = reinterpret_cast<uint32_t *>(jet);
        for (int q = tid; q < FS_JET_ENTRIES * 3 / 4; q += FS_PANEL_THREADS) jdst[q] = jsrc[q];
    }
    __syncthreads();
    // 32-bit indices: a strip has at most 5 * 4096^2 < 2^27 pixels and the grid covers them with less than one block to spare
    const unsigned width = 5u * (unsigned)panel;
    const unsigned pixels = width * (unsigned)panel;
    const unsigned first = (blockIdx.x * FS_PANEL_THREADS + tid) * FS_PANEL_PIXELS_PER_THREAD;
    if (first >= pixels) return;
    uint32_t px[FS_PANEL_PIXELS_PER_THREAD];
    int valid = 0;
#pragma unroll
    for (int j = 0; j < FS_PANEL_PIXELS_PER_THREAD; ++j) {
        const unsigned p = first + j;
        px[j] = 0;
        if (p < pixels) {
            px[j] = fs_strip_pixel(rec, jet, D, S, panel, (int)(p / width), (int)(p % width));
            valid = j + 1;
        }
    }
    fs_store_pixels(out + ((size_t)b * (size_t)pixels + (size_t)first) * 3, px, valid);
}

extern "C" size_t fs_action_panels_work_bytes(int n_actions) {
    if (n_actions < 1) return 0;
    return sizeof(fs_panel_record) * (size_t)n_actions;
}

// one primitive list of fs_action_panels or fs_lane_panels.  owner: "<entry point>: <record>[, lane j]"; of: where the list is
// drawn (" on its <which> panel", or nothing); label: what names a primitive of this list ("<which> ", or nothing)
static bool fs_prims_ok(const int (*prims)[9], int n, const std::string &owner, const std::string &of, const std::string &label) {
    if (n < 0 || n > FS_PANEL_MAX_PRIMS) {
        fs_set_error(owner + " lists " + std::to_string(n) + " primitives" + of + " (0 .. 8)");
        return false;
    }
    for (int q = 0; q < n; ++q) {
        const int *p = prims[q];
        const std::string where = owner + ", " + label + "primitive " + std::to_string(q);
        if (p[0] != FS_PANEL_RING && p[0] != FS_PANEL_SEGMENT) {
            fs_set_error(where + ": unknown kind");
            return false;
        }
        for (int c = 1; c <= 4; ++c)
            if (p[c] < -FS_PANEL_COORD_LIMIT || p[c] > FS_PANEL_COORD_LIMIT) {
                fs_set_error(where + ": |coordinate| above 8191");
                return false;
            }
        if (p[5] < 1 || p[5] > FS_PANEL_THICKNESS_LIMIT) {
            fs_set_error(where + ": thickness outside 1 .. 64");
            return false;
        }
        for (int c = 6; c <= 8; ++c)
            if (p[c] < 0 || p[c] > 255) {
                fs_set_error(where + ": colour outside 0 .. 255");
                return false;
            }
    }
    return true;
}

extern "C" int fs_action_panels(const fs_panel_record *table, int n_actions, int obs_dim, int image_dim, int panel,
                                unsigned char *d_out, void *d_work, void *stream) {
    if (!table || !d_out || !d_work) {
        fs_set_error("fs_action_panels: a null table, output or work buffer");
        return FS_ERR_ARG;
    }
    if (n_actions < 1 || n_actions > 65535) {
        fs_set_error("fs_action_panels: 1 .. 65535 actions per call");
        return FS_ERR_ARG;
    }
    if (obs_dim < 1 || obs_dim > FS_PANEL_LIMIT || image_dim < 1 || image_dim > FS_PANEL_LIMIT || panel < 1 || panel > FS_PANEL_LIMIT) {
        fs_set_error("fs_action_panels: D, S and panel must lie in 1 .. 4096");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_work}) || ((uintptr_t)d_out & 3)) {
        fs_set_error("fs_action_panels: the work buffer must be 16-byte aligned, the output 4-byte aligned");
        return FS_ERR_ARG;
    }
    for (int k = 0; k < n_actions; ++k) {
        const fs_panel_record &r = table[k];
        if (!r.stack || !r.value_map || !r.range || !r.before) {
            fs_set_error("fs_action_panels: action " + std::to_string(k) + " has a null stack, value map, range or before pointer");
            return FS_ERR_ARG;
        }
        if (((uintptr_t)r.stack | (uintptr_t)r.value_map | (uintptr_t)r.range | (uintptr_t)r.before | (uintptr_t)r.after) & 3) {
            fs_set_error("fs_action_panels: action " + std::to_string(k) + " has a pointer off the float grid");
            return FS_ERR_ARG;
        }
        const std::string owner = "fs_action_panels: action " + std::to_string(k);
        if (!fs_prims_ok(r.small, r.n_small, owner, " on its transformed panel", "transformed ") ||
            !fs_prims_ok(r.large, r.n_large, owner, " on its before panel", "before "))
            return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(fs_panel_record) * (size_t)n_actions;
    hipError_t err = hipMemcpyAsync(d_work, table, bytes, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_action_panels upload")) return FS_ERR_HIP;
    const long long pixels = 5LL * panel * panel;
    const long long per_block = (long long)FS_PANEL_THREADS * FS_PANEL_PIXELS_PER_THREAD;
    const unsigned groups = (unsigned)((pixels + per_block - 1) / per_block);   // <= 81920
    hipLaunchKernelGGL(fs_k_action_panels, dim3(groups, (unsigned)n_actions), dim3(FS_PANEL_THREADS), 0, st,
                       (const fs_panel_record *)d_work, obs_dim, image_dim, panel, d_out);
    return fs_hip_ok(hipGetLastError(), "fs_action_panels launch") ? FS_OK : FS_ERR_HIP;
}

// ---- lane strips (flingbot_amd/lookahead.py) ----------------------------------------------------------------------------------
// One strip per look-ahead step and task: the observation before the step with EVERY executed lane's action on it, then the
// observation after each lane.  The rules are fs_action_panels' (quantisation, sampling at the source's resolution, integer
// coverage, one blend with the last covering primitive), plus: a lane's primitives take the lane's rank colour (fs_lane_colours),
// lanes are drawn in rank order, and an after panel is framed in its rank colour, the followed one with a white frame inside it.
// fs_k_lane_panels is fs_k_action_panels with another pixel function: grid (groups of 1024 pixels, records), 256 threads, 4
// consecutive pixels per thread, the record in LDS and read with indices that are the same in the whole workgroup.
#define FS_LANE_COLOUR_VALUES 230, 25, 75, 60, 180, 75, 0, 130, 200, 245, 130, 48, 145, 30, 180, 70, 240, 240, 240, 50, 230, 255, 225, 25

static_assert(sizeof(fs_lane_record) == 2416, "flingbot_amd/report.py LANE_RECORD mirrors this layout");

static const unsigned char fs_lane_colours_host[FS_LANE_MAX * 3] = {FS_LANE_COLOUR_VALUES};
__constant__ unsigned char fs_lane_colours_device[FS_LANE_MAX * 3] = {FS_LANE_COLOUR_VALUES};

extern "C" int fs_lane_colours(unsigned char *out, int n_bytes) {
    if (!out || n_bytes != FS_LANE_MAX * 3) {
        fs_set_error("fs_lane_colours: out must hold 24 bytes");
        return FS_ERR_ARG;
    }
    memcpy(out, fs_lane_colours_host, sizeof(fs_lane_colours_host));
    return FS_OK;
}

// pixel (y, xs) of the lane strip, xs in [0, (1 + lanes) panel): R | G << 8 | B << 16
__device__ __forceinline__ uint32_t fs_lane_pixel(const fs_lane_record &rec, const unsigned char *colours, int S, int panel, int y,
                                                  int xs) {
    const int which = xs / panel, x = xs - which * panel;
    const int sy = (y * S) / panel, sx = (x * S) / panel;
    if (which == 0) {  // the observation with every lane's action: the last lane that covers the pixel, blended once
        const uint32_t base = fs_rgb_at(rec.before, S, sy, sx);
        int hit = -1;
        for (int j = 0; j < rec.n_lanes; ++j)
            for (int k = 0; k < rec.n_prims[j]; ++k)
                if (fs_prim_covers(&rec.prims[j][k][0], sy, sx)) hit = j;
        if (hit < 0) return base;
        const unsigned char *c = colours + 3 * hit;
        const int r = (9 * c[0] + (int)(base & 255) + 5) / 10, g = (9 * c[1] + (int)((base >> 8) & 255) + 5) / 10,
                  b = (9 * c[2] + (int)((base >> 16) & 255) + 5) / 10;
        return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
    }
    const int lane = which - 1;
    if (lane >= rec.n_lanes) return 0u;
    const float *after = rec.after[lane];
    if (!after) return 0u;
    const int t = panel / 50 > 1 ? panel / 50 : 1;
    const int edge = min(min(y, x), min(panel - 1 - y, panel - 1 - x));
    if (edge < t) {
        const unsigned char *c = colours + 3 * lane;
        return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    }
    if (lane == rec.followed && edge < 2 * t) return 0xffffffu;
    return fs_rgb_at(after, S, sy, sx);
}

__global__ __launch_bounds__(FS_PANEL_THREADS) void fs_k_lane_panels(const fs_lane_record *__restrict__ table, int lanes, int S,
                                                                     int panel, unsigned char *__restrict__ out) {
    __shared__ fs_lane_record rec;
    __shared__ unsigned char colours[FS_LANE_MAX * 3];
    const int tid = threadIdx.x, b = blockIdx.y;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(table + b);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&rec);
        for (int q = tid; q < (int)(sizeof(fs_lane_record) / 4); q += FS_PANEL_THREADS) dst[q] = src[q];
        if (tid < FS_LANE_MAX * 3) colours[tid] = fs_lane_colours_device[tid];
    }
    __syncthreads();
    // 32-bit indices: a strip has at most 9 * 4096^2 < 2^28 pixels and the grid covers them with less than one block to spare
    const unsigned width = (unsigned)(1 + lanes) * (unsigned)panel;
    const unsigned pixels = width * (unsigned)panel;
    const unsigned first = (blockIdx.x * FS_PANEL_THREADS + tid) * FS_PANEL_PIXELS_PER_THREAD;
    if (first >= pixels) return;
    uint32_t px[FS_PANEL_PIXELS_PER_THREAD];
    int valid = 0;
#pragma unroll
    for (int j = 0; j < FS_PANEL_PIXELS_PER_THREAD; ++j) {
        const unsigned p = first + j;
        px[j] = 0;
        if (p < pixels) {
            px[j] = fs_lane_pixel(rec, colours, S, panel, (int)(p / width), (int)(p % width));
            valid = j + 1;
        }
    }
    fs_store_pixels(out + ((size_t)b * (size_t)pixels + (size_t)first) * 3, px, valid);
}

extern "C" size_t fs_lane_panels_work_bytes(int n_records) {
    if (n_records < 1) return 0;
    return sizeof(fs_lane_record) * (size_t)n_records;
}

extern "C" int fs_lane_panels(const fs_lane_record *table, int n_records, int lanes, int image_dim, int panel, unsigned char *d_out,
                              void *d_work, void *stream) {
    if (!table || !d_out || !d_work) {
        fs_set_error("fs_lane_panels: a null table, output or work buffer");
        return FS_ERR_ARG;
    }
    if (n_records < 1 || n_records > 65535) {
        fs_set_error("fs_lane_panels: 1 .. 65535 records per call");
        return FS_ERR_ARG;
    }
    if (lanes < 1 || lanes > FS_LANE_MAX) {
        fs_set_error("fs_lane_panels: 1 .. 8 lanes per strip");
        return FS_ERR_ARG;
    }
    if (image_dim < 1 || image_dim > FS_PANEL_LIMIT || panel < 1 || panel > FS_PANEL_LIMIT) {
        fs_set_error("fs_lane_panels: S and panel must lie in 1 .. 4096");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_work}) || ((uintptr_t)d_out & 3)) {
        fs_set_error("fs_lane_panels: the work buffer must be 16-byte aligned, the output 4-byte aligned");
        return FS_ERR_ARG;
    }
    for (int k = 0; k < n_records; ++k) {
        const fs_lane_record &r = table[k];
        const std::string where = "fs_lane_panels: record " + std::to_string(k);
        if (!r.before) {
            fs_set_error(where + " has a null before pointer");
            return FS_ERR_ARG;
        }
        if (r.n_lanes < 1 || r.n_lanes > lanes) {
            fs_set_error(where + " has " + std::to_string(r.n_lanes) + " lanes (1 .. " + std::to_string(lanes) + ")");
            return FS_ERR_ARG;
        }
        if (r.followed < -1 || r.followed >= r.n_lanes) {
            fs_set_error(where + " follows lane " + std::to_string(r.followed) + " (-1 .. " + std::to_string(r.n_lanes - 1) + ")");
            return FS_ERR_ARG;
        }
        uintptr_t bits = (uintptr_t)r.before;
        for (int j = 0; j < r.n_lanes; ++j) bits |= (uintptr_t)r.after[j];
        if (bits & 3) {
            fs_set_error(where + " has a pointer off the float grid");
            return FS_ERR_ARG;
        }
        for (int j = 0; j < r.n_lanes; ++j)
            if (!fs_prims_ok(r.prims[j], r.n_prims[j], where + ", lane " + std::to_string(j), "", "")) return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(fs_lane_record) * (size_t)n_records;
    hipError_t err = hipMemcpyAsync(d_work, table, bytes, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_lane_panels upload")) return FS_ERR_HIP;
    const long long pixels = (1LL + lanes) * panel * panel;
    const long long per_block = (long long)FS_PANEL_THREADS * FS_PANEL_PIXELS_PER_THREAD;
    const unsigned groups = (unsigned)((pixels + per_block - 1) / per_block);   // <= 147456
    hipLaunchKernelGGL(fs_k_lane_panels, dim3(groups, (unsigned)n_records), dim3(FS_PANEL_THREADS), 0, st,
                       (const fs_lane_record *)d_work, lanes, image_dim, panel, d_out);
    return fs_hip_ok(hipGetLastError(), "fs_lane_panels launch") ? FS_OK : FS_ERR_HIP;
}

// ---- probe strips (flingbot_amd/probe.py) -------------------------------------------------------------------------------------
// One strip per probed map: what the net saw with the chosen action | the predicted map | the measured map on its lattice | the
// observation after the best-measured cell.  Panels 0, 1 and 3 are fs_action_panels' panels 2, 1 and 4 (the same functions);
// panel 2 colours a map pixel by the lattice cell it is nearest to.  fs_k_probe_panels is fs_k_action_panels with another
// pixel function: grid (groups of 1024 pixels, records), 256 threads, 4 consecutive pixels per thread, the record in LDS.
static_assert(sizeof(fs_probe_record) == 368, "flingbot_amd/report.py PROBE_RECORD mirrors this layout");

// pixel (y, xs) of the probe strip, xs in [0, 4 panel): R | G << 8 | B << 16
__device__ __forceinline__ uint32_t fs_probe_pixel(const fs_probe_record &rec, const unsigned char *jet, int D, int S, int panel,
                                                   int y, int xs) {
    const int which = xs / panel, x = xs - which * panel;
    if (which == 3) return rec.after ? fs_rgb_at(rec.after, S, (y * S) / panel, (x * S) / panel) : 0u;
    const int sy = (y * D) / panel, sx = (x * D) / panel;
    if (which == 0) {
        const uint32_t base = fs_rgb_at(rec.stack, D, sy, sx);
        return fs_overlay(&rec.small[0][0], rec.n_small, sy, sx, base & 255, (base >> 8) & 255, (base >> 16) & 255);
    }
    if (which == 1) return fs_value_colour(jet, rec.value_map[(size_t)sy * D + sx], rec.range[0], rec.range[1]);
    const int ny = sy - rec.y0 + rec.stride / 2, nz = sx - rec.z0 + rec.stride / 2;
    if (ny < 0 || nz < 0) return 0u;
    const int i = ny / rec.stride, j = nz / rec.stride;
    if (i >= rec.gy || j >= rec.gz) return 0u;
    if (i == rec.cy && j == rec.cz) {   // the chosen cell's outermost source pixels
        const int ry = ny - i * rec.stride, rz = nz - j * rec.stride;
        if (ry == 0 || rz == 0 || ry == rec.stride - 1 || rz == rec.stride - 1) return 0xffffffu;
    }
    const float m = rec.measured[(size_t)i * rec.gz + j];
    if (__builtin_isfinite(m)) return fs_value_colour(jet, m, rec.range[0], rec.range[1]);
    return (rec.code[(size_t)i * rec.gz + j] & 1) ? 0x808080u : 0x404040u;   // valid but not executed / invalid
}

__global__ __launch_bounds__(FS_PANEL_THREADS) void fs_k_probe_panels(const fs_probe_record *__restrict__ table, int D, int S,
                                                                      int panel, unsigned char *__restrict__ out) {
    __shared__ fs_probe_record rec;
    __shared__ unsigned char jet[FS_JET_ENTRIES * 3];
    const int tid = threadIdx.x, b = blockIdx.y;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(table + b);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&rec);
        for (int q = tid; q < (int)(sizeof(fs_probe_record) / 4); q += FS_PANEL_THREADS) dst[q] = src[q];
        const uint32_t *jsrc = reinterpret_cast<const uint32_t *>(fs_jet_device);
        uint32_t *jdst = reinterpret_cast<uint32_t *>(jet);
        for (int q = tid; q < FS_JET_ENTRIES * 3 / 4; q += FS_PANEL_THREADS) jdst[q] = jsrc[q];
    }
    __syncthreads();
    // 32-bit indices: a strip has at most 4 * 4096^2 = 2^26 pixels and the grid covers them with less than one block to spare
    const unsigned width = 4u * (unsigned)panel;
    const unsigned pixels = width * (unsigned)panel;
    const unsigned first = (blockIdx.x * FS_PANEL_THREADS + tid) * FS_PANEL_PIXELS_PER_THREAD;
    if (first >= pixels) return;
    uint32_t px[FS_PANEL_PIXELS_PER_THREAD];
    int valid = 0;
#pragma unroll
    for (int j = 0; j < FS_PANEL_PIXELS_PER_THREAD; ++j) {
        const unsigned p = first + j;
        px[j] = 0;
        if (p < pixels) {
            px[j] = fs_probe_pixel(rec, jet, D, S, panel, (int)(p / width), (int)(p % width));
            valid = j + 1;
        }
    }
    fs_store_pixels(out + ((size_t)b * (size_t)pixels + (size_t)first) * 3, px, valid);
}

extern "C" size_t fs_probe_panels_work_bytes(int n_records) {
    if (n_records < 1) return 0;
    return sizeof(fs_probe_record) * (size_t)n_records;
}

extern "C" int fs_probe_panels(const fs_probe_record *table, int n_records, int obs_dim, int image_dim, int panel,
                               unsigned char *d_out, void *d_work, void *stream) {
    if (!table || !d_out || !d_work) {
        fs_set_error("fs_probe_panels: a null table, output or work buffer");
        return FS_ERR_ARG;
    }
    if (n_records < 1 || n_records > 65535) {
        fs_set_error("fs_probe_panels: 1 .. 65535 records per call");
        return FS_ERR_ARG;
    }
    if (obs_dim < 1 || obs_dim > FS_PANEL_LIMIT || image_dim < 1 || image_dim > FS_PANEL_LIMIT || panel < 1 || panel > FS_PANEL_LIMIT) {
        fs_set_error("fs_probe_panels: D, S and panel must lie in 1 .. 4096");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_work}) || ((uintptr_t)d_out & 3)) {
        fs_set_error("fs_probe_panels: the work buffer must be 16-byte aligned, the output 4-byte aligned");
        return FS_ERR_ARG;
    }
    for (int k = 0; k < n_records; ++k) {
        const fs_probe_record &r = table[k];
        const std::string where = "fs_probe_panels: record " + std::to_string(k);
        if (!r.stack || !r.value_map || !r.range || !r.measured || !r.code) {
            fs_set_error(where + " has a null stack, value map, range, measured or code pointer");
            return FS_ERR_ARG;
        }
        if (((uintptr_t)r.stack | (uintptr_t)r.value_map | (uintptr_t)r.range | (uintptr_t)r.measured | (uintptr_t)r.after) & 3) {
            fs_set_error(where + " has a pointer off the float grid");
            return FS_ERR_ARG;
        }
        if (r.stride < 1 || r.gy < 1 || r.gz < 1 || (long long)r.gy * r.gz > 4096) {
            fs_set_error(where + ": stride below 1 or gy * gz outside 1 .. 4096");
            return FS_ERR_ARG;
        }
        if (r.y0 < 0 || r.z0 < 0 || r.y0 + (long long)(r.gy - 1) * r.stride >= obs_dim ||
            r.z0 + (long long)(r.gz - 1) * r.stride >= obs_dim) {
            fs_set_error(where + ": the lattice leaves the map");
            return FS_ERR_ARG;
        }
        if (r.cy < -1 || r.cy >= r.gy || r.cz < -1 || r.cz >= r.gz) {
            fs_set_error(where + ": the chosen cell is outside the lattice (-1: none)");
            return FS_ERR_ARG;
        }
        if (!fs_prims_ok(r.small, r.n_small, where, " on its transformed panel", "")) return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(fs_probe_record) * (size_t)n_records;
    hipError_t err = hipMemcpyAsync(d_work, table, bytes, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_probe_panels upload")) return FS_ERR_HIP;
    const long long pixels = 4LL * panel * panel;
    const long long per_block = (long long)FS_PANEL_THREADS * FS_PANEL_PIXELS_PER_THREAD;
    const unsigned groups = (unsigned)((pixels + per_block - 1) / per_block);   // <= 65536
    hipLaunchKernelGGL(fs_k_probe_panels, dim3(groups, (unsigned)n_records), dim3(FS_PANEL_THREADS), 0, st,
                       (const fs_probe_record *)d_work, obs_dim, image_dim, panel, d_out);
    return fs_hip_ok(hipGetLastError(), "fs_probe_panels launch") ? FS_OK : FS_ERR_HIP;
}
