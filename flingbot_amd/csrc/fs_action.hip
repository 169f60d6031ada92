// fs_action.hip -- device-side action selection.
//
// Reference: SimEnv.get_max_value_valid_action (environment/simEnv.py:560-661) sorts all P*T*(D-2g)^2 value-map entries
// (221 184 for FlingBot's 96 x 48 x 48) on the CPU and walks them in descending order, running per candidate
// get_action_params (:517-537), pixels_to_3d_positions (environment/utils.py:237-276: transform-matrix product,
// truncation to pretransform pixels, bounds, two depth look-ups + unprojection) and the arm reachability test
// (:539-558, stretchdrag's end points :624-642) until one passes.  Here every candidate is validated in parallel with the
// same float64 expressions and the answer is one masked arg-max: highest value among the valid candidates, lowest
// flattened index among equals -- exactly the candidate the reference's walk stops at.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flingsim.h"
#include "fs_context.h"

struct FsActionCfg {
    int P, T, D, S, g, drag, place;
    int kind[FS_ACTION_MAX_PRIMITIVES];  // FS_ACTION_FLING ...
    double fx, cx;                       // compute_intrinsics: focal length, principal point (= S / 2)
    double pose[16];                     // compute_pose(...) row-major
    double left[3], right[3];
    double reach, stretchdrag_dist, grasp_height;
};

__device__ __forceinline__ bool fs_act_unproject(const FsActionCfg &c, const float *depth, int x, int y, double *out) {
    const double z = (double)depth[(size_t)y * c.S + x];  // depth_im[y, x]
    if (z == 0.0) return false;                           // the reference raises 'Invalid pick point'
    const double px = ((double)x - c.cx) * z / c.fx;
    const double py = ((double)y - c.cx) * z / c.fx;
    for (int i = 0; i < 3; ++i) out[i] = c.pose[4 * i] * px + c.pose[4 * i + 1] * py + c.pose[4 * i + 2] * z + c.pose[4 * i + 3] * 1.0;
    out[0] = -out[0];
    return true;
}

__device__ __forceinline__ bool fs_act_reach(const FsActionCfg &c, const double *base, const double *p) {
    const double dx = base[0] - p[0], dy = base[1] - p[1], dz = base[2] - p[2];
    return sqrt(dx * dx + dy * dy + dz * dz) < c.reach;
}

// validity of candidate (primitive p, transform t, pixel (y, z) in the D x D map)
__device__ bool fs_act_valid(const FsActionCfg &c, const double *mats, const float *depth, int p, int t, int y, int z) {
    const int kind = c.kind[p];
    int a0, a1, b0, b1;  // reach points (row, column) in the transformed image
    if (kind == FS_ACTION_FLING || kind == FS_ACTION_STRETCHDRAG) { a0 = y + c.g; a1 = z; b0 = y - c.g; b1 = z; }
    else if (kind == FS_ACTION_DRAG) { a0 = y; a1 = z; b0 = y + c.drag; b1 = z; }
    else { a0 = y; a1 = z; b0 = y + c.place; b1 = z; }
    if (a0 < 0 || a1 < 0 || b0 < 0 || b1 < 0 || a0 >= c.D || a1 >= c.D || b0 >= c.D || b1 >= c.D) return false;
    const double *m = mats + 9 * (size_t)t;  // get_transform_matrix(S, D, -rotation, scale), row-major
    // np.matmul([[a0, a1, 1], [b0, b1, 1]], mat)[:, :2].astype(int)
    const int pa0 = (int)((double)a0 * m[0] + (double)a1 * m[3] + 1.0 * m[6]);
    const int pa1 = (int)((double)a0 * m[1] + (double)a1 * m[4] + 1.0 * m[7]);
    const int pb0 = (int)((double)b0 * m[0] + (double)b1 * m[3] + 1.0 * m[6]);
    const int pb1 = (int)((double)b0 * m[1] + (double)b1 * m[4] + 1.0 * m[7]);
    if (pa0 < 0 || pa1 < 0 || pb0 < 0 || pb1 < 0 || pa0 >= c.S || pa1 >= c.S || pb0 >= c.S || pb1 >= c.S) return false;
    double P1[3], P2[3];
    if (!fs_act_unproject(c, depth, pa0, pa1, P1) || !fs_act_unproject(c, depth, pb0, pb1, P2)) return false;
    bool reachable;
    if (kind == FS_ACTION_FLING || kind == FS_ACTION_STRETCHDRAG)
        reachable = fs_act_reach(c, c.left, P1) && fs_act_reach(c, c.right, P2);
    else
        reachable = (fs_act_reach(c, c.left, P1) && fs_act_reach(c, c.left, P2)) ||
                    (fs_act_reach(c, c.right, P1) && fs_act_reach(c, c.right, P2));
    if (kind == FS_ACTION_STRETCHDRAG) {
        P1[1] = c.grasp_height; P2[1] = c.grasp_height;
        const double e0 = P1[0] - P2[0], e1 = P1[1] - P2[1], e2 = P1[2] - P2[2];
        // np.cross(e, [0, 1, 0])
        double d0 = e1 * 0.0 - e2 * 1.0, d1 = e2 * 0.0 - e0 * 0.0, d2 = e0 * 1.0 - e1 * 0.0;
        const double nrm = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        d0 = c.stretchdrag_dist * d0 / nrm; d1 = c.stretchdrag_dist * d1 / nrm; d2 = c.stretchdrag_dist * d2 / nrm;
        const double L[3] = {P1[0] + d0, P1[1] + d1, P1[2] + d2}, R[3] = {P2[0] + d0, P2[1] + d1, P2[2] + d2};
        reachable = (fs_act_reach(c, c.left, L) && fs_act_reach(c, c.right, R)) && reachable;
    }
    return reachable;
}

struct FsActionBest { float val; long long idx; };

__device__ __forceinline__ bool fs_act_better(float v, long long i, float bv, long long bi) {
    return bi < 0 || v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(256) void fs_k_action_scan(const float *values, const float *depth, const double *mats,
                                                        FsActionCfg c, FsActionBest *block_best) {
    __shared__ float sv[256];
    __shared__ long long si[256];
    const int W = c.D - 2 * c.g;
    const long long total = (long long)c.P * c.T * W * W;
    float bv = 0.0f;
    long long bi = -1;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
        const int zz = (int)(k % W), yy = (int)((k / W) % W);
        const int t = (int)((k / ((long long)W * W)) % c.T), p = (int)(k / ((long long)W * W * c.T));
        const int y = yy + c.g, z = zz + c.g;
        const float v = values[(((size_t)p * c.T + t) * c.D + y) * c.D + z];
        if (!(v == v)) continue;                      // NaN never equals a sorted value in the reference's walk
        if (!fs_act_better(v, k, bv, bi)) continue;   // cannot win: skip the validity work
        if (fs_act_valid(c, mats, depth, p, t, y, z)) { bv = v; bi = k; }
    }
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const long long oi = si[threadIdx.x + s];
            if (oi >= 0 && fs_act_better(sv[threadIdx.x + s], oi, sv[threadIdx.x], si[threadIdx.x])) {
                sv[threadIdx.x] = sv[threadIdx.x + s];
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { block_best[blockIdx.x].val = sv[0]; block_best[blockIdx.x].idx = si[0]; }
}

__global__ __launch_bounds__(256) void fs_k_action_final(const FsActionBest *block_best, int n_blocks, FsActionBest *out) {
    __shared__ float sv[256];
    __shared__ long long si[256];
    float bv = 0.0f;
    long long bi = -1;
    for (int b = threadIdx.x; b < n_blocks; b += blockDim.x) {
        const FsActionBest x = block_best[b];
        if (x.idx >= 0 && fs_act_better(x.val, x.idx, bv, bi)) { bv = x.val; bi = x.idx; }
    }
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const long long oi = si[threadIdx.x + s];
            if (oi >= 0 && fs_act_better(sv[threadIdx.x + s], oi, sv[threadIdx.x], si[threadIdx.x])) {
                sv[threadIdx.x] = sv[threadIdx.x + s];
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out->val = sv[0]; out->idx = si[0]; }
}

#define FS_ACTION_BLOCKS 1024

extern "C" size_t fs_select_action_work_bytes(int n_transforms) {
    if (n_transforms < 0) return 0;
    return sizeof(double) * 9 * (size_t)n_transforms + sizeof(FsActionBest) * (FS_ACTION_BLOCKS + 1) + 512;
}

extern "C" int fs_select_action(const float *d_values, int n_primitives, const int *primitive_kinds, int n_transforms,
                                int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist,
                                const double *transform_mats, const float *d_depth, int depth_dim, double focal_length,
                                const double *pose_matrix, const double *left_arm_base, const double *right_arm_base,
                                double reach_distance_limit, double stretchdrag_dist, double grasp_height,
                                long long *best_index_out, float *best_value_out, void *d_work, void *stream) {
    if (!d_values || !primitive_kinds || !transform_mats || !d_depth || !pose_matrix || !left_arm_base || !right_arm_base ||
        !best_index_out || !d_work || n_primitives <= 0 || n_primitives > FS_ACTION_MAX_PRIMITIVES || n_transforms <= 0 ||
        obs_dim <= 2 * pix_grasp_dist || pix_grasp_dist < 0 || depth_dim <= 0) {
        fs_set_error("fs_select_action: bad arguments");
        return FS_ERR_ARG;
    }
    FsActionCfg c;
    memset(&c, 0, sizeof(c));
    c.P = n_primitives; c.T = n_transforms; c.D = obs_dim; c.S = depth_dim;
    c.g = pix_grasp_dist; c.drag = pix_drag_dist; c.place = pix_place_dist;
    for (int p = 0; p < n_primitives; ++p) {
        if (primitive_kinds[p] < FS_ACTION_FLING || primitive_kinds[p] > FS_ACTION_PLACE) {
            fs_set_error("fs_select_action: unknown primitive kind");
            return FS_ERR_ARG;
        }
        c.kind[p] = primitive_kinds[p];
    }
    c.fx = focal_length; c.cx = (double)depth_dim / 2.0;
    memcpy(c.pose, pose_matrix, sizeof(c.pose));
    memcpy(c.left, left_arm_base, sizeof(c.left));
    memcpy(c.right, right_arm_base, sizeof(c.right));
    c.reach = reach_distance_limit; c.stretchdrag_dist = stretchdrag_dist; c.grasp_height = grasp_height;
    hipStream_t st = (hipStream_t)stream;
    double *d_mats = (double *)d_work;
    FsActionBest *d_best = (FsActionBest *)((char *)d_work + ((sizeof(double) * 9 * (size_t)n_transforms + 255) & ~(size_t)255));
    hipError_t err = hipMemcpyAsync(d_mats, transform_mats, sizeof(double) * 9 * (size_t)n_transforms, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_select_action upload")) return FS_ERR_HIP;
    const int W = obs_dim - 2 * pix_grasp_dist;
    const long long total = (long long)n_primitives * n_transforms * W * W;
    int blocks = (int)((total + 255) / 256);
    if (blocks > FS_ACTION_BLOCKS) blocks = FS_ACTION_BLOCKS;
    hipLaunchKernelGGL(fs_k_action_scan, dim3(blocks), dim3(256), 0, st, d_values, d_depth, d_mats, c, d_best);
    hipLaunchKernelGGL(fs_k_action_final, dim3(1), dim3(256), 0, st, d_best, blocks, d_best + FS_ACTION_BLOCKS);
    FsActionBest h;
    err = hipMemcpyAsync(&h, d_best + FS_ACTION_BLOCKS, sizeof(h), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (!fs_hip_ok(err, "fs_select_action download")) return FS_ERR_HIP;
    *best_index_out = h.idx;
    if (best_value_out) *best_value_out = h.val;
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fs_transform_winners: the same masked arg-max, reduced per (episode, primitive, transform) map instead of over everything,
// for n episodes in one launch.  Neighbouring pixels of one map have near-equal values, so the K best PIXELS of an observation
// are K copies of one action; the winners of distinct rotation x scale maps are different actions (flingbot_amd/lookahead.py).
// One workgroup per map: a thread walks its pixels in ascending order and keeps the first best valid one, the workgroup
// reduces in LDS with fs_select_action's own order (higher value, then lower index).  fs_act_valid is used as it is.
__global__ __launch_bounds__(256) void fs_k_transform_winners(const float *values, const float *depth, const double *mats,
                                                              FsActionCfg c, FsActionBest *out) {
    __shared__ float sv[256];
    __shared__ long long si[256];
    const int W = c.D - 2 * c.g;
    const int map = blockIdx.x;                      // ((episode * P) + p) * T + t
    const int t = map % c.T, p = (map / c.T) % c.P, e = map / (c.T * c.P);
    const float *vmap = values + (size_t)map * c.D * c.D;
    const float *edepth = depth + (size_t)e * c.S * c.S;
    const double *emats = mats + (size_t)e * c.T * 9;
    const long long first = (long long)(p * c.T + t) * W * W;  // the map's first entry in the episode's flattened index
    float bv = 0.0f;
    long long bi = -1;
    for (int k = threadIdx.x; k < W * W; k += blockDim.x) {
        const int yy = k / W, zz = k - yy * W;
        const int y = yy + c.g, z = zz + c.g;
        const float v = vmap[(size_t)y * c.D + z];
        if (!(v == v)) continue;                              // NaN is skipped, as in fs_k_action_scan
        if (!fs_act_better(v, first + k, bv, bi)) continue;   // cannot win: skip the validity work
        if (fs_act_valid(c, emats, edepth, p, t, y, z)) { bv = v; bi = first + k; }
    }
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const long long oi = si[threadIdx.x + s];
            if (oi >= 0 && fs_act_better(sv[threadIdx.x + s], oi, sv[threadIdx.x], si[threadIdx.x])) {
                sv[threadIdx.x] = sv[threadIdx.x + s];
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[map].val = sv[0]; out[map].idx = si[0]; }
}

static size_t fs_winners_mats_bytes(int n, int n_transforms) {
    return (sizeof(double) * 9 * (size_t)n * (size_t)n_transforms + 255) & ~(size_t)255;
}

extern "C" size_t fs_transform_winners_work_bytes(int n, int n_primitives, int n_transforms) {
    if (n <= 0 || n_primitives <= 0 || n_transforms <= 0) return 0;
    return fs_winners_mats_bytes(n, n_transforms) + sizeof(FsActionBest) * (size_t)n * n_primitives * n_transforms + 256;
}

extern "C" int fs_transform_winners(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                                    int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist,
                                    const double *transform_mats, const float *d_depth, int depth_dim, double focal_length,
                                    const double *pose_matrix, const double *left_arm_base, const double *right_arm_base,
                                    double reach_distance_limit, double stretchdrag_dist, double grasp_height,
                                    long long *index_out, float *value_out, void *d_work, void *stream) {
    if (!d_values || !primitive_kinds || !transform_mats || !d_depth || !pose_matrix || !left_arm_base || !right_arm_base ||
        !index_out || !value_out || !d_work || n <= 0 || n > 65536 || n_primitives <= 0 ||
        n_primitives > FS_ACTION_MAX_PRIMITIVES || n_transforms <= 0 || n_transforms > 4096 || obs_dim <= 2 * pix_grasp_dist ||
        obs_dim > 4096 || pix_grasp_dist < 0 || depth_dim <= 0 || depth_dim > 16384) {
        fs_set_error("fs_transform_winners: bad arguments");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_work})) { fs_set_error("fs_transform_winners: d_work must be 16-byte aligned"); return FS_ERR_ARG; }
    FsActionCfg c;
    memset(&c, 0, sizeof(c));
    c.P = n_primitives; c.T = n_transforms; c.D = obs_dim; c.S = depth_dim;
    c.g = pix_grasp_dist; c.drag = pix_drag_dist; c.place = pix_place_dist;
    for (int p = 0; p < n_primitives; ++p) {
        if (primitive_kinds[p] < FS_ACTION_FLING || primitive_kinds[p] > FS_ACTION_PLACE) {
            fs_set_error("fs_transform_winners: unknown primitive kind");
            return FS_ERR_ARG;
        }
        c.kind[p] = primitive_kinds[p];
    }
    c.fx = focal_length; c.cx = (double)depth_dim / 2.0;
    memcpy(c.pose, pose_matrix, sizeof(c.pose));
    memcpy(c.left, left_arm_base, sizeof(c.left));
    memcpy(c.right, right_arm_base, sizeof(c.right));
    c.reach = reach_distance_limit; c.stretchdrag_dist = stretchdrag_dist; c.grasp_height = grasp_height;
    hipStream_t st = (hipStream_t)stream;
    const size_t maps = (size_t)n * n_primitives * n_transforms;
    if (maps > (size_t)1 << 24) { fs_set_error("fs_transform_winners: more than 2^24 maps in one call"); return FS_ERR_ARG; }
    double *d_mats = (double *)d_work;
    FsActionBest *d_best = (FsActionBest *)((char *)d_work + fs_winners_mats_bytes(n, n_transforms));
    hipError_t err = hipMemcpyAsync(d_mats, transform_mats, sizeof(double) * 9 * (size_t)n * n_transforms, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_transform_winners upload")) return FS_ERR_HIP;
    hipLaunchKernelGGL(fs_k_transform_winners, dim3((unsigned)maps), dim3(256), 0, st, d_values, d_depth, d_mats, c, d_best);
    std::vector<FsActionBest> h(maps);
    err = hipMemcpyAsync(h.data(), d_best, sizeof(FsActionBest) * maps, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (!fs_hip_ok(err, "fs_transform_winners download")) return FS_ERR_HIP;
    for (size_t k = 0; k < maps; ++k) { index_out[k] = h[k].idx; value_out[k] = h[k].idx >= 0 ? h[k].val : 0.0f; }
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fs_lattice_actions: the validity test per CELL instead of behind a reduction -- a lattice of pixels of chosen maps, each
// cell with its validity (fs_act_valid as it is), the two on-cloth bits of BatchedFlingEnv._on_cloth and the map's value
// (flingbot_amd/probe.py executes the valid cells of one map side by side).  One workgroup per request, cells strided
// over its threads.
__device__ bool fs_act_on_cloth(const float *depth, int S, int col, int row, int r) {
    // every pixel of the plane inside the disc dy^2 + dx^2 <= r^2 around (row, col), clipped to the image, is cloth
    const int y0 = row - r < 0 ? 0 : row - r, y1 = row + r > S - 1 ? S - 1 : row + r;
    const int x0 = col - r < 0 ? 0 : col - r, x1 = col + r > S - 1 ? S - 1 : col + r;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const int dy = y - row, dx = x - col;
            if (dy * dy + dx * dx <= r * r && depth[(size_t)y * S + x] == 2.0f) return false;
        }
    return true;
}

__global__ __launch_bounds__(256) void fs_k_lattice_actions(const float *values, const float *depth, const double *mats,
                                                            FsActionCfg c, const fs_lattice_request *requests, int pitch,
                                                            int radius, unsigned char *code_out, float *value_out) {
    const fs_lattice_request q = requests[blockIdx.x];
    const float *vmap = values + (((size_t)q.episode * c.P + q.primitive) * c.T + q.transform) * c.D * c.D;
    const float *edepth = depth + (size_t)q.episode * c.S * c.S;
    const double *emats = mats + (size_t)q.episode * c.T * 9;
    for (int k = threadIdx.x; k < pitch; k += blockDim.x) {
        unsigned char code = 0;
        float v = 0.0f;
        if (k < q.gy * q.gz) {
            const int i = k / q.gz, j = k - i * q.gz;
            const int y = q.y0 + i * q.stride, z = q.z0 + j * q.stride;
            v = vmap[(size_t)y * c.D + z];
            if (fs_act_valid(c, emats, edepth, q.primitive, q.transform, y, z)) {
                // the reach points once more (fs_act_valid keeps them to itself): the same expressions, inside the image
                const int kind = c.kind[q.primitive];
                int a0 = y, b0 = y + c.place;
                if (kind == FS_ACTION_FLING || kind == FS_ACTION_STRETCHDRAG) { a0 = y + c.g; b0 = y - c.g; }
                else if (kind == FS_ACTION_DRAG) b0 = y + c.drag;
                const double *m = emats + 9 * (size_t)q.transform;
                const int pa0 = (int)((double)a0 * m[0] + (double)z * m[3] + 1.0 * m[6]);
                const int pa1 = (int)((double)a0 * m[1] + (double)z * m[4] + 1.0 * m[7]);
                const int pb0 = (int)((double)b0 * m[0] + (double)z * m[3] + 1.0 * m[6]);
                const int pb1 = (int)((double)b0 * m[1] + (double)z * m[4] + 1.0 * m[7]);
                code = 1;
                if (radius <= 0 || fs_act_on_cloth(edepth, c.S, pa0, pa1, radius)) code |= 2;   // depth_im[pa1, pa0]: column pa0
                if (radius <= 0 || fs_act_on_cloth(edepth, c.S, pb0, pb1, radius)) code |= 4;
            }
        }
        code_out[(size_t)blockIdx.x * pitch + k] = code;   // (cells past a smaller request's lattice: 0 / 0.0f)
        value_out[(size_t)blockIdx.x * pitch + k] = v;
    }
}

static size_t fs_round256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t fs_lattice_actions_work_bytes(int n, int n_transforms, int m, int max_cells) {
    if (n <= 0 || n_transforms <= 0 || m <= 0 || max_cells <= 0) return 0;
    return fs_winners_mats_bytes(n, n_transforms) + fs_round256(sizeof(fs_lattice_request) * (size_t)m) +
           fs_round256(sizeof(float) * (size_t)m * max_cells) + fs_round256((size_t)m * max_cells) + 256;
}

extern "C" int fs_lattice_actions(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                                  int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist,
                                  const double *transform_mats, const float *d_depth, int depth_dim, double focal_length,
                                  const double *pose_matrix, const double *left_arm_base, const double *right_arm_base,
                                  double reach_distance_limit, double stretchdrag_dist, double grasp_height,
                                  const fs_lattice_request *requests, int m, int conservative_grasp_radius,
                                  unsigned char *code_out, float *value_out, void *d_work, void *stream) {
    if (!d_values || !primitive_kinds || !transform_mats || !d_depth || !pose_matrix || !left_arm_base || !right_arm_base ||
        !requests || !code_out || !value_out || !d_work || n <= 0 || n > 65536 || n_primitives <= 0 ||
        n_primitives > FS_ACTION_MAX_PRIMITIVES || n_transforms <= 0 || n_transforms > 4096 || obs_dim <= 2 * pix_grasp_dist ||
        obs_dim > 4096 || pix_grasp_dist < 0 || depth_dim <= 0 || depth_dim > 16384) {
        fs_set_error("fs_lattice_actions: bad arguments");
        return FS_ERR_ARG;
    }
    if (m < 1 || m > 65535) { fs_set_error("fs_lattice_actions: the number of requests must be 1 .. 65535"); return FS_ERR_ARG; }
    if (fs_misaligned16({d_work})) { fs_set_error("fs_lattice_actions: d_work must be 16-byte aligned"); return FS_ERR_ARG; }
    int pitch = 0;
    for (int k = 0; k < m; ++k) {
        const fs_lattice_request &q = requests[k];
        if (q.episode < 0 || q.episode >= n || q.primitive < 0 || q.primitive >= n_primitives || q.transform < 0 ||
            q.transform >= n_transforms) {
            fs_set_error("fs_lattice_actions: a request's episode, primitive or transform is out of range");
            return FS_ERR_ARG;
        }
        if (q.stride < 1) { fs_set_error("fs_lattice_actions: a request's stride must be at least 1"); return FS_ERR_ARG; }
        if (q.gy < 1 || q.gz < 1 || (long long)q.gy * q.gz > 4096) {
            fs_set_error("fs_lattice_actions: a request's gy * gz must be 1 .. 4096");
            return FS_ERR_ARG;
        }
        if (q.y0 < 0 || q.z0 < 0 || q.y0 + (long long)(q.gy - 1) * q.stride >= obs_dim ||
            q.z0 + (long long)(q.gz - 1) * q.stride >= obs_dim) {
            fs_set_error("fs_lattice_actions: a request's lattice leaves the map");
            return FS_ERR_ARG;
        }
        if (q.gy * q.gz > pitch) pitch = q.gy * q.gz;
    }
    FsActionCfg c;
    memset(&c, 0, sizeof(c));
    c.P = n_primitives; c.T = n_transforms; c.D = obs_dim; c.S = depth_dim;
    c.g = pix_grasp_dist; c.drag = pix_drag_dist; c.place = pix_place_dist;
    for (int p = 0; p < n_primitives; ++p) {
        if (primitive_kinds[p] < FS_ACTION_FLING || primitive_kinds[p] > FS_ACTION_PLACE) {
            fs_set_error("fs_lattice_actions: unknown primitive kind");
            return FS_ERR_ARG;
        }
        c.kind[p] = primitive_kinds[p];
    }
    c.fx = focal_length; c.cx = (double)depth_dim / 2.0;
    memcpy(c.pose, pose_matrix, sizeof(c.pose));
    memcpy(c.left, left_arm_base, sizeof(c.left));
    memcpy(c.right, right_arm_base, sizeof(c.right));
    c.reach = reach_distance_limit; c.stretchdrag_dist = stretchdrag_dist; c.grasp_height = grasp_height;
    // a disc of radius 2 S covers the image from any of its pixels: larger radii mean the same and would overflow r * r
    const int radius = conservative_grasp_radius > 2 * depth_dim ? 2 * depth_dim : conservative_grasp_radius;
    hipStream_t st = (hipStream_t)stream;
    // one table: the matrices, then the requests (staged together, one upload)
    const size_t mats_bytes = fs_winners_mats_bytes(n, n_transforms), req_bytes = fs_round256(sizeof(fs_lattice_request) * (size_t)m);
    const size_t val_bytes = fs_round256(sizeof(float) * (size_t)m * pitch);
    std::vector<char> table(mats_bytes + req_bytes, 0);
    memcpy(table.data(), transform_mats, sizeof(double) * 9 * (size_t)n * n_transforms);
    memcpy(table.data() + mats_bytes, requests, sizeof(fs_lattice_request) * (size_t)m);
    char *base = (char *)d_work;
    float *d_val = (float *)(base + mats_bytes + req_bytes);
    unsigned char *d_code = (unsigned char *)(base + mats_bytes + req_bytes + val_bytes);
    hipError_t err = hipMemcpyAsync(base, table.data(), table.size(), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_lattice_actions upload")) return FS_ERR_HIP;
    hipLaunchKernelGGL(fs_k_lattice_actions, dim3((unsigned)m), dim3(256), 0, st, d_values, d_depth, (const double *)base, c,
                       (const fs_lattice_request *)(base + mats_bytes), pitch, radius, d_code, d_val);
    // the two planes lie back to back: one download
    std::vector<char> h(val_bytes + (size_t)m * pitch);
    err = hipMemcpyAsync(h.data(), d_val, h.size(), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (!fs_hip_ok(err, "fs_lattice_actions download")) return FS_ERR_HIP;
    memcpy(value_out, h.data(), sizeof(float) * (size_t)m * pitch);
    memcpy(code_out, h.data() + val_bytes, (size_t)m * pitch);
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fs_sample_actions: K distinct valid actions per observation, drawn without replacement with probability proportional to
// exp(value / tau) -- Gumbel-top-K: every candidate gets ONE perturbed key, value * inv_tau + noise[hash(candidate, key)], and
// the K largest keys are the draw (include/flingsim.h has the rules).  Two launches:
//   fs_k_sample_keys    every candidate of every observation once: fs_act_valid (the float64 part), the on-cloth bit and the
//                       key, into a float and a byte per candidate of d_work.
//   fs_k_sample_rounds  one workgroup per observation runs the k rounds.  A round is a scan over the observation's bytes (four
//                       candidates per 32-bit word, the keys behind them as one float4) that keeps the best candidate not
//                       suppressed by an earlier pick, a shuffle / LDS arg-max in the order (key descending, index ascending),
//                       and thread 0 appending the pick to the LDS list the next round's suppression test reads.
// An observation's rows are padded to a multiple of 16 candidates so that the word and float4 loads stay aligned.
#define FS_SAMPLE_MAX_K 16
#define FS_SAMPLE_THREADS 1024
#define FS_SAMPLE_VALID 1     // the value is not NaN and fs_act_valid holds: what a greedy pick may take
#define FS_SAMPLE_DRAW 2      // ... and the grasp points are on cloth (where asked) and the key is not NaN: a sampled pick

struct FsSampleCfg {
    int k, first_greedy, on_cloth, radius, separation;
    float inv_tau;
    long long total, stride;  // candidates of one observation; its padded row length
};

__device__ __forceinline__ unsigned int fs_sample_hash(unsigned int c, unsigned int key_lo, unsigned int key_hi) {
    unsigned int h = c * 0x9E3779B1u + key_lo * 0x85EBCA77u + key_hi * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}

// the pretransform pixel pair of a candidate: fs_act_valid's expressions once more (it keeps them to itself)
__device__ __forceinline__ void fs_sample_pixels(const FsActionCfg &c, const double *m, int kind, int y, int z, int *pix) {
    int a0 = y, b0 = y + c.place;
    if (kind == FS_ACTION_FLING || kind == FS_ACTION_STRETCHDRAG) { a0 = y + c.g; b0 = y - c.g; }
    else if (kind == FS_ACTION_DRAG) b0 = y + c.drag;
    pix[0] = (int)((double)a0 * m[0] + (double)z * m[3] + 1.0 * m[6]);
    pix[1] = (int)((double)a0 * m[1] + (double)z * m[4] + 1.0 * m[7]);
    pix[2] = (int)((double)b0 * m[0] + (double)z * m[3] + 1.0 * m[6]);
    pix[3] = (int)((double)b0 * m[1] + (double)z * m[4] + 1.0 * m[7]);
}

struct FsSampleWhere { int p, t, y, z; };

__device__ __forceinline__ FsSampleWhere fs_sample_decode(const FsActionCfg &c, int W, int k) {
    FsSampleWhere w;
    const int zz = k % W, r = k / W, yy = r % W, m = r / W;
    w.t = m % c.T; w.p = m / c.T; w.y = yy + c.g; w.z = zz + c.g;
    return w;
}

__global__ __launch_bounds__(256) void fs_k_sample_keys(const float *values, const float *depth, const double *mats,
                                                        const unsigned int *sample_keys, const float *noise, FsActionCfg c,
                                                        FsSampleCfg s, int blocks_per_obs, float *key_out,
                                                        unsigned char *flag_out) {
    const int e = blockIdx.x / blocks_per_obs;
    const long long k = (long long)(blockIdx.x - e * blocks_per_obs) * blockDim.x + threadIdx.x;
    if (k >= s.stride) return;
    unsigned char flag = 0;
    float key = 0.0f;
    if (k < s.total) {
        const int W = c.D - 2 * c.g;
        const FsSampleWhere w = fs_sample_decode(c, W, (int)k);
        const float v = values[((((size_t)e * c.P + w.p) * c.T + w.t) * c.D + w.y) * c.D + w.z];
        const float *edepth = depth + (size_t)e * c.S * c.S;
        const double *emats = mats + (size_t)e * c.T * 9;
        if (v == v && fs_act_valid(c, emats, edepth, w.p, w.t, w.y, w.z)) {
            flag = FS_SAMPLE_VALID;
            const int kind = c.kind[w.p];
            bool cloth = true;
            if (s.on_cloth && s.radius > 0) {
                int pix[4];
                fs_sample_pixels(c, emats + 9 * (size_t)w.t, kind, w.y, w.z, pix);
                cloth = fs_act_on_cloth(edepth, c.S, pix[0], pix[1], s.radius);   // depth_im[pix[1], pix[0]]: column pix[0]
                if (cloth && (kind == FS_ACTION_FLING || kind == FS_ACTION_STRETCHDRAG))
                    cloth = fs_act_on_cloth(edepth, c.S, pix[2], pix[3], s.radius);
            }
            const unsigned int h = fs_sample_hash((unsigned int)k, sample_keys[2 * e], sample_keys[2 * e + 1]);
            key = __fadd_rn(__fmul_rn(v, s.inv_tau), noise[h >> 16]);   // two roundings: never one fused multiply-add
            if (cloth && key == key) flag |= FS_SAMPLE_DRAW;
        }
    }
    key_out[(size_t)e * s.stride + k] = key;
    flag_out[(size_t)e * s.stride + k] = flag;
}

struct FsSamplePick { int prim, pix[4]; };

__device__ __forceinline__ bool fs_sample_better(float x, int i, float bx, int bi) {
    return bi < 0 || x > bx || (x == bx && i < bi);
}

__device__ __forceinline__ bool fs_sample_suppressed(const FsActionCfg &c, const double *emats, int W, int k,
                                                     const FsSamplePick *picks, int n_picks, int separation) {
    const FsSampleWhere w = fs_sample_decode(c, W, k);
    bool same = false;
    for (int j = 0; j < n_picks; ++j) same = same || picks[j].prim == w.p;
    if (!same) return false;
    int pix[4];
    fs_sample_pixels(c, emats + 9 * (size_t)w.t, c.kind[w.p], w.y, w.z, pix);
    for (int j = 0; j < n_picks; ++j) {
        if (picks[j].prim != w.p) continue;
        bool near = true;
        for (int q = 0; q < 4; ++q) {
            const int d = pix[q] - picks[j].pix[q];
            near = near && (d < 0 ? -d : d) <= separation;
        }
        if (near) return true;
    }
    return false;
}

__global__ __launch_bounds__(FS_SAMPLE_THREADS) void fs_k_sample_rounds(const float *values, const double *mats, FsActionCfg c,
                                                                        FsSampleCfg s, const float *keys,
                                                                        const unsigned char *flags, long long *index_out,
                                                                        float *value_out, float *key_out, int *pix_out) {
    __shared__ float sx[FS_SAMPLE_THREADS / 64];
    __shared__ int si[FS_SAMPLE_THREADS / 64];
    __shared__ FsSamplePick picks[FS_SAMPLE_MAX_K];
    __shared__ int s_found;
    const int e = blockIdx.x, W = c.D - 2 * c.g;
    const float *evalues = values + (size_t)e * c.P * c.T * c.D * c.D;
    const double *emats = mats + (size_t)e * c.T * 9;
    const float *ekeys = keys + (size_t)e * s.stride;
    const unsigned char *eflags = flags + (size_t)e * s.stride;
    const int stride = (int)s.stride;
    int pick = 0;
    for (; pick < s.k; ++pick) {
        const bool greedy = s.first_greedy && pick == 0;
        const unsigned int want = greedy ? FS_SAMPLE_VALID : FS_SAMPLE_DRAW;
        float bx = 0.0f;
        int bi = -1;
        // a thread's candidates come in ascending order: an equal key never replaces what it holds
        for (int k4 = threadIdx.x * 4; k4 < stride; k4 += FS_SAMPLE_THREADS * 4) {
            const unsigned int word = *(const unsigned int *)(eflags + k4);
            if (!(word & (want * 0x01010101u))) continue;
            const float4 kv = *(const float4 *)(ekeys + k4);
            const float x4[4] = {kv.x, kv.y, kv.z, kv.w};
            for (int j = 0; j < 4; ++j) {
                if (!((word >> (8 * j)) & want)) continue;
                const int k = k4 + j;
                float x = x4[j];
                if (greedy) {
                    const FsSampleWhere w = fs_sample_decode(c, W, k);
                    x = evalues[(((size_t)w.p * c.T + w.t) * c.D + w.y) * c.D + w.z];
                }
                if (bi >= 0 && !(x > bx)) continue;
                if (pick > 0 && fs_sample_suppressed(c, emats, W, k, picks, pick, s.separation)) continue;
                bx = x; bi = k;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ox = __shfl_down(bx, off, 64);
            const int oi = __shfl_down(bi, off, 64);
            if (oi >= 0 && fs_sample_better(ox, oi, bx, bi)) { bx = ox; bi = oi; }
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { sx[wave] = bx; si[wave] = bi; }
        __syncthreads();
        if (wave == 0) {
            bx = lane < FS_SAMPLE_THREADS / 64 ? sx[lane] : 0.0f;
            bi = lane < FS_SAMPLE_THREADS / 64 ? si[lane] : -1;
            for (int off = FS_SAMPLE_THREADS / 128; off > 0; off >>= 1) {
                const float ox = __shfl_down(bx, off, 64);
                const int oi = __shfl_down(bi, off, 64);
                if (oi >= 0 && fs_sample_better(ox, oi, bx, bi)) { bx = ox; bi = oi; }
            }
            if (lane == 0) {
                s_found = bi;
                if (bi >= 0) {
                    const FsSampleWhere w = fs_sample_decode(c, W, bi);
                    FsSamplePick got;
                    got.prim = w.p;
                    fs_sample_pixels(c, emats + 9 * (size_t)w.t, c.kind[w.p], w.y, w.z, got.pix);
                    picks[pick] = got;
                    const size_t o = (size_t)e * s.k + pick;
                    index_out[o] = bi;
                    value_out[o] = evalues[(((size_t)w.p * c.T + w.t) * c.D + w.y) * c.D + w.z];
                    key_out[o] = bx;
                    for (int q = 0; q < 4; ++q) pix_out[4 * o + q] = got.pix[q];
                }
            }
        }
        __syncthreads();
        if (s_found < 0) break;   // the picks only grow: what found nothing now finds nothing later
    }
    for (int j = pick + (int)threadIdx.x; j < s.k; j += FS_SAMPLE_THREADS) {
        const size_t o = (size_t)e * s.k + j;
        index_out[o] = -1; value_out[o] = 0.0f; key_out[o] = 0.0f;
        for (int q = 0; q < 4; ++q) pix_out[4 * o + q] = 0;
    }
}

// the shapes fs_sample_actions takes: the candidates of one observation, 0 where they are refused
static long long fs_sample_total(int n, int n_primitives, int n_transforms, int obs_dim, int pix_grasp_dist, int k) {
    if (n <= 0 || n > 65536 || n_primitives <= 0 || n_primitives > FS_ACTION_MAX_PRIMITIVES || n_transforms <= 0 ||
        n_transforms > 4096 || pix_grasp_dist < 0 || obs_dim <= 2 * pix_grasp_dist || obs_dim > 4096 || k < 1 || k > FS_SAMPLE_MAX_K)
        return 0;
    const long long W = obs_dim - 2 * pix_grasp_dist, total = (long long)n_primitives * n_transforms * W * W;
    return total < (1LL << 31) - 16 ? total : 0;
}

static long long fs_sample_stride(long long total) { return (total + 15) & ~15LL; }

extern "C" size_t fs_sample_actions_work_bytes(int n, int n_primitives, int n_transforms, int obs_dim, int pix_grasp_dist, int k) {
    const long long total = fs_sample_total(n, n_primitives, n_transforms, obs_dim, pix_grasp_dist, k);
    if (total <= 0) return 0;
    const size_t cells = (size_t)n * (size_t)fs_sample_stride(total);
    return fs_winners_mats_bytes(n, n_transforms) + fs_round256(sizeof(unsigned int) * 2 * (size_t)n) +
           fs_round256(sizeof(float) * cells) + fs_round256(cells) + fs_round256(32 * (size_t)n * k) + 256;
}

extern "C" int fs_sample_actions(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                                 int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist,
                                 const double *transform_mats, const float *d_depth, int depth_dim, double focal_length,
                                 const double *pose_matrix, const double *left_arm_base, const double *right_arm_base,
                                 double reach_distance_limit, double stretchdrag_dist, double grasp_height, int k,
                                 const float *d_noise, int noise_bits, float inv_tau, const unsigned int *sample_keys,
                                 int first_greedy, int on_cloth, int conservative_grasp_radius, int separation,
                                 long long *index_out, float *value_out, float *key_out, int *pix_out, void *d_work,
                                 void *stream) {
    if (!d_values || !primitive_kinds || !transform_mats || !d_depth || !pose_matrix || !left_arm_base || !right_arm_base ||
        !d_noise || !sample_keys || !index_out || !value_out || !key_out || !pix_out || !d_work) {
        fs_set_error("fs_sample_actions: a null pointer");
        return FS_ERR_ARG;
    }
    if (k < 1 || k > FS_SAMPLE_MAX_K) { fs_set_error("fs_sample_actions: k must be 1 .. 16"); return FS_ERR_ARG; }
    if (noise_bits != 16) { fs_set_error("fs_sample_actions: noise_bits must be 16"); return FS_ERR_ARG; }
    if (!std::isfinite(inv_tau) || inv_tau < 0.0f) {
        fs_set_error("fs_sample_actions: inv_tau must be finite and not negative");
        return FS_ERR_ARG;
    }
    if (separation < 0) { fs_set_error("fs_sample_actions: separation must not be negative"); return FS_ERR_ARG; }
    if ((first_greedy != 0 && first_greedy != 1) || (on_cloth != 0 && on_cloth != 1)) {
        fs_set_error("fs_sample_actions: first_greedy and on_cloth are 0 or 1");
        return FS_ERR_ARG;
    }
    if (n <= 0 || n > 65536 || n_primitives <= 0 || n_primitives > FS_ACTION_MAX_PRIMITIVES || n_transforms <= 0 ||
        n_transforms > 4096 || obs_dim <= 2 * pix_grasp_dist || obs_dim > 4096 || pix_grasp_dist < 0 || depth_dim <= 0 ||
        depth_dim > 16384) {
        fs_set_error("fs_sample_actions: bad arguments");
        return FS_ERR_ARG;
    }
    const long long total = fs_sample_total(n, n_primitives, n_transforms, obs_dim, pix_grasp_dist, k);
    if (total <= 0) { fs_set_error("fs_sample_actions: 2^31 candidates or more per observation"); return FS_ERR_ARG; }
    const long long stride = fs_sample_stride(total);
    const long long blocks_per_obs = (stride + 255) / 256;
    if (blocks_per_obs * n >= (1LL << 31)) { fs_set_error("fs_sample_actions: too many candidates in one call"); return FS_ERR_ARG; }
    if (fs_misaligned16({d_work})) { fs_set_error("fs_sample_actions: d_work must be 16-byte aligned"); return FS_ERR_ARG; }
    FsActionCfg c;
    memset(&c, 0, sizeof(c));
    c.P = n_primitives; c.T = n_transforms; c.D = obs_dim; c.S = depth_dim;
    c.g = pix_grasp_dist; c.drag = pix_drag_dist; c.place = pix_place_dist;
    for (int p = 0; p < n_primitives; ++p) {
        if (primitive_kinds[p] < FS_ACTION_FLING || primitive_kinds[p] > FS_ACTION_PLACE) {
            fs_set_error("fs_sample_actions: unknown primitive kind");
            return FS_ERR_ARG;
        }
        c.kind[p] = primitive_kinds[p];
    }
    c.fx = focal_length; c.cx = (double)depth_dim / 2.0;
    memcpy(c.pose, pose_matrix, sizeof(c.pose));
    memcpy(c.left, left_arm_base, sizeof(c.left));
    memcpy(c.right, right_arm_base, sizeof(c.right));
    c.reach = reach_distance_limit; c.stretchdrag_dist = stretchdrag_dist; c.grasp_height = grasp_height;
    FsSampleCfg s;
    s.k = k; s.first_greedy = first_greedy; s.on_cloth = on_cloth; s.separation = separation; s.inv_tau = inv_tau;
    s.total = total; s.stride = stride;
    // a disc of radius 2 S covers the image from any of its pixels: larger radii mean the same and would overflow r * r
    s.radius = conservative_grasp_radius > 2 * depth_dim ? 2 * depth_dim : conservative_grasp_radius;
    hipStream_t st = (hipStream_t)stream;
    // one table: the matrices, then the keys (staged together, one upload)
    const size_t mats_bytes = fs_winners_mats_bytes(n, n_transforms), tbl_bytes = fs_round256(sizeof(unsigned int) * 2 * (size_t)n);
    const size_t cells = (size_t)n * (size_t)stride, picks = (size_t)n * k;
    std::vector<char> table(mats_bytes + tbl_bytes, 0);
    memcpy(table.data(), transform_mats, sizeof(double) * 9 * (size_t)n * n_transforms);
    memcpy(table.data() + mats_bytes, sample_keys, sizeof(unsigned int) * 2 * (size_t)n);
    char *base = (char *)d_work;
    const double *d_mats = (const double *)base;
    const unsigned int *d_tbl = (const unsigned int *)(base + mats_bytes);
    float *d_keys = (float *)(base + mats_bytes + tbl_bytes);
    unsigned char *d_flags = (unsigned char *)d_keys + fs_round256(sizeof(float) * cells);
    char *d_out = (char *)d_flags + fs_round256(cells);
    long long *d_index = (long long *)d_out;              // [picks] int64, then value, key float32 [picks], pixels int32 [picks][4]
    float *d_value = (float *)(d_out + 8 * picks), *d_key = (float *)(d_out + 12 * picks);
    int *d_pix = (int *)(d_out + 16 * picks);
    hipError_t err = hipMemcpyAsync(base, table.data(), table.size(), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable source
    if (!fs_hip_ok(err, "fs_sample_actions upload")) return FS_ERR_HIP;
    hipLaunchKernelGGL(fs_k_sample_keys, dim3((unsigned)(blocks_per_obs * n)), dim3(256), 0, st, d_values, d_depth, d_mats, d_tbl,
                       d_noise, c, s, (int)blocks_per_obs, d_keys, d_flags);
    hipLaunchKernelGGL(fs_k_sample_rounds, dim3((unsigned)n), dim3(FS_SAMPLE_THREADS), 0, st, d_values, d_mats, c, s,
                       (const float *)d_keys, (const unsigned char *)d_flags, d_index, d_value, d_key, d_pix);
    std::vector<char> h(32 * picks);
    err = hipMemcpyAsync(h.data(), d_out, h.size(), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (!fs_hip_ok(err, "fs_sample_actions download")) return FS_ERR_HIP;
    memcpy(index_out, h.data(), 8 * picks);
    memcpy(value_out, h.data() + 8 * picks, 4 * picks);
    memcpy(key_out, h.data() + 12 * picks, 4 * picks);
    memcpy(pix_out, h.data() + 16 * picks, 16 * picks);
    return FS_OK;
}
