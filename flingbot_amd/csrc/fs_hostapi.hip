// fs_hostapi.hip -- host-only entry points of the C-ABI (no HIP device needed): scene builder and camera set-up.
// They let the CPU test-suite check the host logic (bit-exact topology, camera matrices) without a GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flingsim.h"
#include "fs_context.h"
#include "fs_camera.h"
#include "fs_sphere_mesh.h"
#include "fs_pair_search.h"

struct fs_host_scene { FsHostScene s; };  // (same definition in fs_capi.hip: fs_set_scene_prebuilt)

extern "C" fs_host_scene *fs_host_scene_build(const float *scene_params, int n_params, const float *verts,
                                              int n_vert_floats, const int *stretch, int n_stretch_ints, const int *bend,
                                              int n_bend_ints, const int *shear, int n_shear_ints, const int *faces,
                                              int n_face_ints) {
    fs_host_scene *h = new fs_host_scene();
    std::string err = fs_build_scene(h->s, scene_params, n_params, verts, n_vert_floats, stretch, n_stretch_ints, bend,
                                     n_bend_ints, shear, n_shear_ints, faces, n_face_ints);
    if (!err.empty()) {
        fs_set_error(err);
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void fs_host_scene_free(fs_host_scene *h) { delete h; }
extern "C" int fs_host_scene_counts(const fs_host_scene *h, int *n, int *m, int *t, int *max_deg) {
    if (!h) return FS_ERR_ARG;
    if (n) *n = h->s.n;
    if (m) *m = h->s.m;
    if (t) *t = h->s.t;
    if (max_deg) *max_deg = h->s.max_deg;
    return FS_OK;
}
extern "C" int fs_host_scene_copy(const fs_host_scene *h, int what, void *out, int n_elems) {
    if (!h || !out) return FS_ERR_ARG;
    const FsHostScene &s = h->s;
    const void *src = nullptr;
    size_t count = 0;
    FsParams p = s.params;
    float packed[32];
    switch (what) {
        case FS_SCENE_POSITIONS: src = s.pos.data(); count = s.pos.size(); break;
        case FS_SCENE_VELOCITIES: src = s.vel.data(); count = s.vel.size(); break;
        case FS_SCENE_PHASES: src = s.phase.data(); count = s.phase.size(); break;
        case FS_SCENE_SPRINGS: src = s.springs.data(); count = s.springs.size(); break;
        case FS_SCENE_SPRING_LENGTHS: src = s.spring_len.data(); count = s.spring_len.size(); break;
        case FS_SCENE_SPRING_STIFFNESS: src = s.spring_k.data(); count = s.spring_k.size(); break;
        case FS_SCENE_TRIANGLES: src = s.tris.data(); count = s.tris.size(); break;
        case FS_SCENE_TRI_NORMALS: src = s.tri_normals.data(); count = s.tri_normals.size(); break;
        case FS_SCENE_ADJ_OFFSETS: src = s.adj_off.data(); count = s.adj_off.size(); break;
        case FS_SCENE_ADJ_NEIGHBORS: src = s.adj_j.data(); count = s.adj_j.size(); break;
        case FS_SCENE_BOUNDS: {
            if (n_elems < 6) { fs_set_error("buffer too small"); return FS_ERR_ARG; }
            memcpy(out, s.scene_lower, 12);
            memcpy((char *)out + 12, s.scene_upper, 12);
            return FS_OK;
        }
        case FS_SCENE_PARAMS: {
            if (n_elems < 32) { fs_set_error("buffer too small"); return FS_ERR_ARG; }
            memset(packed, 0, sizeof(packed));
            packed[0] = (float)p.numIterations; packed[1] = (float)p.numSubsteps; packed[2] = p.dt;
            packed[3] = p.gravity[0]; packed[4] = p.gravity[1]; packed[5] = p.gravity[2];
            packed[6] = p.radius; packed[7] = p.solidRestDistance; packed[8] = p.collisionDistance;
            packed[9] = p.shapeCollisionMargin; packed[10] = p.particleCollisionMargin; packed[11] = p.dynamicFriction;
            packed[12] = p.staticFriction; packed[13] = p.particleFriction; packed[14] = p.damping;
            packed[15] = p.sleepThreshold; packed[16] = p.relaxationFactor; packed[17] = p.maxAcceleration;
            packed[18] = p.maxSpeed; packed[19] = p.restitution; packed[20] = p.adhesion; packed[21] = p.dissipation;
            packed[22] = (float)p.numPlanes; packed[23] = p.planes[0][0]; packed[24] = p.planes[0][1];
            packed[25] = p.planes[0][2]; packed[26] = p.planes[0][3]; packed[27] = (float)p.maxNeighbors;
            packed[28] = (float)p.maxContacts; packed[29] = (float)p.relaxationMode;
            memcpy(out, packed, sizeof(packed));
            return FS_OK;
        }
        case FS_SCENE_FLAGS: {
            if (n_elems < 4) { fs_set_error("buffer too small"); return FS_ERR_ARG; }
            const int flags[4] = {s.restnear_ok, s.g64_ok, s.gp_L_ok, s.gp_halvable};
            memcpy(out, flags, sizeof(flags));
            return FS_OK;
        }
        case FS_SCENE_RESTNEAR: src = s.restnear_w.data(); count = s.restnear_ok ? s.restnear_w.size() : 0; break;
        case FS_SCENE_STREAM_CODES: src = s.scode.data(); count = s.sdict_size > 0 ? s.scode.size() : 0; break;
        case FS_SCENE_STREAM_DICT: src = s.sdict.data(); count = s.sdict_size > 0 ? (size_t)4 * s.sdict_size : 0; break;
        // the packed mesh words: these two selectors RETURN the number of elements copied (0 = the cloth has no words, mesh_ok == 0)
        case FS_SCENE_MESH_WORDS: src = s.mesh_w.data(); count = s.mesh_ok ? s.mesh_w.size() : 0; break;
        case FS_SCENE_MESH_STIFFNESS: src = s.mesh_k; count = s.mesh_ok ? 4 : 0; break;
        default: fs_set_error("unknown scene array id"); return FS_ERR_ARG;
    }
    if ((size_t)n_elems < count) { fs_set_error("buffer too small"); return FS_ERR_ARG; }
    if (count) memcpy(out, src, count * 4);   // (an empty array -- the springs of a 1 x 1 cloth -- has no data pointer to copy from)
    if (what == FS_SCENE_MESH_WORDS || what == FS_SCENE_MESH_STIFFNESS) return (int)count;
    return FS_OK;
}

// RenderScene's camera / light set-up (main.cpp:1411-1438): out[0:16] view, [16:32] proj, [32:48] lightTransform
// (all row-major, column-vector convention), [48:51] lightPos, [51:54] lightDir.
extern "C" int fs_camera_matrices(const float *cam_pos3, const float *cam_angle3, int width, int height,
                                  const float *scene_lower3, const float *scene_upper3, float *out54) {
    if (!cam_pos3 || !cam_angle3 || !scene_lower3 || !scene_upper3 || !out54 || width <= 0 || height <= 0) return FS_ERR_ARG;
    FsRasterFrame fr;
    fs_raster_setup(fr, cam_pos3, cam_angle3, width, height, scene_lower3, scene_upper3);
    memcpy(out54, fr.view, 64);
    memcpy(out54 + 16, fr.proj, 64);
    memcpy(out54 + 32, fr.light_vp, 64);
    memcpy(out54 + 48, fr.light_pos, 12);
    memcpy(out54 + 51, fr.light_dir, 12);
    return FS_OK;
}

// The mesh fs_render rasterises for ONE kinematic sphere, computed by the same functions on the host
// (fs_raster_kernels.h: fs_sphere_trig, fs_quat_axes, fs_sphere_vertex, fs_sphere_tri) = what the reference draws
// (core/mesh.cpp:858-902 + main.cpp:1739-1751).  verts / normals: float[4 * 441], tris: int[3 * 800]; each may be null.
extern "C" int fs_host_sphere_mesh(float radius, const float *prev_pos3, const float *prev_quat4, float *verts,
                                   float *normals, int *tris) {
    if (!prev_pos3 || !prev_quat4) return FS_ERR_ARG;
    FsSphereTrig trig;
    fs_sphere_trig(trig);
    float a[9];
    fs_quat_axes(prev_quat4, a);
    for (int v = 0; v < FS_SPHERE_VERTS; ++v) {
        FsVec4 p, n;
        fs_sphere_vertex(trig, a, radius, prev_pos3[0], prev_pos3[1], prev_pos3[2], v, p, n);
        if (verts) memcpy(verts + 4 * v, &p, 16);
        if (normals) memcpy(normals + 4 * v, &n, 16);
    }
    if (tris)
        for (int t = 0; t < FS_SPHERE_TRIS; ++t) fs_sphere_tri(t, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]);
    return FS_OK;
}

// The half-stencil neighbour search of fs_k_fused_grid64 (find mode 4) on the host: the rule of fs_pair_search.h on given
// positions (float[4 * n], xyzw) with a hash of 2^bucket_bits buckets.  dimx > 0 applies the stencil filter of a canonical
// grid cloth of that width (the 8 grid neighbours are no candidates); dimx = 0 keeps every pair.  counts[n], lists[n][ncap]
// (ascending ids, the ncap smallest), facts[4] = {hits the visit-row test rejected (hash aliases), runs that wrapped around
// the end of the bucket table, particles over the cap, longest list before truncation}.
extern "C" int fs_host_pair_search(int n, const float *pos4, float radius, int bucket_bits, int ncap, int dimx, int *counts,
                                   int *lists, int *facts) {
    if (n < 0 || ncap <= 0 || bucket_bits < 2 || bucket_bits > 16 || !(radius > 0.0f) || dimx < 0 ||
        (n > 0 && (!pos4 || !counts || !lists))) {
        fs_set_error("fs_host_pair_search: bad arguments");
        return FS_ERR_ARG;
    }
    const float rad2 = radius * radius, inv_rad = 1.0f / radius;
    const int nb = 1 << bucket_bits;
    std::vector<int> cell(3 * (size_t)n), bucket(n), cursor(nb, 0), items(n);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) cell[3 * i + k] = (int)floorf(pos4[4 * i + k] * inv_rad);
        bucket[i] = (fs_pair_row(cell[3 * i + 1], cell[3 * i + 2], bucket_bits) + cell[3 * i]) & (nb - 1);
        ++cursor[bucket[i]];
    }
    // histogram -> exclusive scan -> scatter; afterwards cursor[b] = end of bucket b, as in the kernel
    for (int b = 0, run = 0; b < nb; ++b) { const int c = cursor[b]; cursor[b] = run; run += c; }
    for (int i = 0; i < n; ++i) items[cursor[bucket[i]]++] = i;
    std::vector<std::vector<int>> found(n);
    int alias_hits = 0, wrapped = 0;
    for (int qs = 0; qs < n; ++qs) {
        const int i = items[qs];
        const float *xi = pos4 + 4 * i;
        const int *ci = &cell[3 * i];
        for (int r = 0; r < FS_PAIR_RUNS; ++r)
            for (int seg = 0; seg < 2; ++seg) {
                int beg, end;
                if (!fs_pair_run_segment(cursor.data(), bucket_bits, r, seg, qs, ci[0], ci[1], ci[2], beg, end)) break;
                if (seg == 1) ++wrapped;
                for (int s = beg; s < end; ++s) {
                    const int j = items[s];
                    const float *xj = pos4 + 4 * j;
                    const float ex = xi[0] - xj[0], ey = xi[1] - xj[1], ez = xi[2] - xj[2];
                    const float d2 = ex * ex + ey * ey + ez * ez;
                    if (!(d2 < rad2)) continue;
                    const int *cj = &cell[3 * j];
                    if (!fs_pair_run_takes(r, cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2])) { ++alias_hits; continue; }
                    if (dimx > 0) {
                        const int ri = i / dimx, rj = j / dimx;
                        if ((unsigned)(rj - ri + 1) <= 2u && (unsigned)((j - rj * dimx) - (i - ri * dimx) + 1) <= 2u) continue;
                    }
                    found[i].push_back(j);
                    found[j].push_back(i);
                }
            }
    }
    int over = 0, longest = 0;
    for (int i = 0; i < n; ++i) {
        std::vector<int> &f = found[i];
        std::sort(f.begin(), f.end());
        const int len = (int)f.size();
        if (len > longest) longest = len;
        if (len > ncap) ++over;
        counts[i] = len < ncap ? len : ncap;
        for (int k = 0; k < ncap; ++k) lists[(size_t)i * ncap + k] = k < len ? f[k] : -1;
    }
    if (facts) { facts[0] = alias_hits; facts[1] = wrapped; facts[2] = over; facts[3] = longest; }
    return FS_OK;
}
