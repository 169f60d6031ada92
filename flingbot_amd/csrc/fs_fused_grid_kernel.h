// fs_fused_grid_kernel.h -- fused LDS-resident solver, specialised for grid cloths that are 64 particles wide.
//
// Same frame structure, same arithmetic and the same bits as fs_k_fused_step (fs_fused_kernel.h: one 1024-thread
// workgroup per episode, predict -> hash -> two-phase neighbour search -> contact set -> 30 Jacobi iterations ->
// finalize, everything resident in LDS); what changes is how the SPRINGS of an iteration are evaluated -- 2/3 of the
// VALU instructions of the frame.  A 64-wide grid maps one cloth ROW onto one wavefront (lane = column), and the
// reference's task sizes make the 64 x 64 cloth the one that fits this kernel (environment/tasks.py:108-121: sides
// 64..104), so that case gets its own code:
//
//   * No adjacency.  The neighbour of slot s is (column + dx_s, row + dz_s) of the canonical CreateSpringGrid list
//     (FS_G64_DX_LIST / FS_G64_DZ_LIST, helpers.h:838-924; the host verifies the cloth against it): dz is an IMMEDIATE
//     offset of the LDS read, dx one of five address registers.  The 24 adjacency dwords per particle and iteration,
//     their registers and their address arithmetic are gone.
//   * Positions are SoA planes in LDS (x | y | z | invMass, 16 KiB each).  In the iterations the thread's particles are
//     rows 2w, 2w+1, 2w+32, 2w+33 (FG_ROW); adjacent rows are 256 B apart, so ONE ds_read2st64_b32 returns the same
//     neighbour slot of TWO of the thread's particles (P, Q) in a register PAIR: 36 LDS instructions per pair of
//     particles and iteration instead of 2 x 24, conflict-free (each half reads one row).
//   * Two particles per trip as TWO INDEPENDENT SCALAR STREAMS (fg_scale / fg_accum on .x = P and .y = Q): the whole spring
//     (difference, length^2, the hardware reciprocal root v_rsq_f32, scale, accumulation) is evaluated for both, bit for bit the
//     operations of fs_spring_fast in the same order per particle, and each stream fills the other's dependency stalls.
//     (The register pairs are also the operand shape of v_pk_add/mul/fma_f32, and the kernel was first written on those:
//     bit-identical and 14 % slower -- a packed multiply / add costs 1.5-1.7 scalar ones on this part, scripts/ubench --
//     so the packed form is NOT what ships; EXPERIMENTS.md "packed fp32".)
//   * A spring between two particles of the same wave and trip (the horizontal ones of P and Q, the vertical and diagonal ones
//     between them) is evaluated ONCE, by the endpoint whose slot comes first in the canonical order s0..s11 -- s0, s1 of P
//     and Q, Q's s2, s3, s8 -- and the partner's slot further down the chain (s4, s5; P's s6, s7, s10) takes the scale through
//     a DPP lane shift or the same thread: 17 reciprocal roots per trip instead of 24, every neighbour gathered once, every
//     difference taken once (DESIGN 4.1 has the table).
//   * No per-spring bookkeeping.  A slot that leaves the grid gets stiffness 0 (its scale becomes +-0, which leaves
//     the accumulators untouched), the constraint count of a particle is its number of in-grid slots, and the
//     `length > 0` test of fs_spring -- false only for coincident particles -- is a minimum over the squared lengths
//     checked once per pair; if it ever fires, or a wave sees a neighbour of different mass (picked particle), the pair
//     takes the exact general path (ELL adjacency, fs_spring).
// Rest lengths: x-direction slots depend on the column only (a 512 B LDS table: slots 0 and 1, the only x-direction ones
// evaluated), z-direction ones on the row only (a 1 KiB LDS table), shear ones per particle (6 loads per trip, from L2,
// issued well ahead of their use) -- verified by the host (build_grid64) because CreateSpringGrid takes them from the fp32
// particle positions.
// Stiffness: the `stiffness / 2, or +0 outside the grid` of an evaluated slot is table data as well -- per column for the
// shear slots (FG_OFF_KS), per row for the z-direction ones (FG_OFF_KZ) -- read through the addresses of the rest-length
// tables with immediate offsets, so a column or z edge costs no compare, select or scalar-register traffic inside the trip
// (the ROW condition of a shear slot is one compare and one address select per pair of slots: rows of +0 in the pad).
#pragma once
#include "fs_fused_kernel.h"

#define FG_PLANE (FS_FUSED_MAX_PARTICLES * 4)  // bytes of one coordinate plane
#define FG_PAD 1024                            // rows -2, -1 of the gathers of the first cloth rows land here (finite zeros); its
                                               // four rows of +0 are also the stiffness of a shear slot whose ROW leaves the grid
#define FG_OFF_XX FG_PAD
#define FG_OFF_X0 (FG_OFF_XX + 4 * FG_PLANE)   // X0x | X0y | X0z (bucket-ordered predicted positions during the search)
#define FG_OFF_CACC (FG_OFF_X0 + 3 * FG_PLANE)  // accumulators of the contact set, 16 B each; the overflow queue's follow without a
                                               // gap (in the idle hash tables), so slot s of either is entry s of ONE array
#define FG_OFF_CUR (FG_OFF_CACC + FS_FUSED_CSET_CAP * 16)
#define FG_OFF_ITEMS (FG_OFF_CUR + FS_FUSED_CUR_BYTES)
#define FG_OFF_SCAN (FG_OFF_ITEMS + FS_FUSED_MAX_PARTICLES * 2)
#define FG_OFF_CSET (FG_OFF_SCAN + 64)
#define FG_OFF_CHIST (FG_OFF_CSET + FS_FUSED_CSET_CAP * 2)
#define FG_OFF_ROWL (FG_OFF_CHIST + 512)       // float[4][64]: rest length of the z-direction slots 8..11 per row
#define FG_OFF_KZ (FG_OFF_ROWL + 1024)         // float[4][64]: stiffness / 2 of the z-direction slots 8..11 per row (+0 where row + dz
                                               // leaves the grid)
#define FG_OFF_KS (FG_OFF_KZ + 1024)           // float[4][64]: stiffness / 2 of the shear slots 2, 3, 6, 7 per column (+0 where column + dx does)
#define FG_OFF_COLL (FG_OFF_KS + 1024)         // float[2][64]: rest length of the x-direction slots 0, 1 per column
#define FG_OFF_RCNT (FG_OFF_COLL + 512)        // float[128]: relaxationFactor / count, the IEEE quotient fs_apply computes
#define FG_LDS_BYTES (FG_OFF_RCNT + 512)
static_assert(FG_OFF_ROWL % 8 == 0 && (FG_OFF_KZ - FG_OFF_ROWL) % 8 == 0, "row tables are read as ds_read_b64 pairs");
static_assert((FG_OFF_COLL - FG_OFF_KS) % 256 == 0, "column tables share one address, rows as ds_read2st64_b32 offsets");
static_assert(FG_LDS_BYTES <= 160 * 1024, "grid-64 kernel: the LDS of one CU");
static_assert(FG_OFF_CACC % 16 == 0 && FG_OFF_CUR == FG_OFF_CACC + FS_FUSED_CSET_CAP * 16, "set and queue accumulators: one array");
// An iteration is three block-wide phases, a barrier after each:
//   spring phase   every wave sums the springs of its four rows, two rows per trip.  A particle with a slot in the contact set
//                  or the overflow queue parks {spring sums, spring count} in the slot's accumulator; every other particle keeps
//                  them in registers named per trip, P and Q side by side (counts packed 8 bits each): one rotation of six
//                  registers between the two trips, none inside a trip.
//   contact phase  thread e of the set / lane q of the queue adds the particle contacts of its particle, in list order, to the
//                  parked sums and writes them back.  Nothing else: no shapes, no applyDeltas, no new position.
//   finish phase   every thread finishes its own four particles, each exactly once and every lane of every wave busy, a trip's
//                  P and Q in one body: sums from the slot or the registers, planes, spheres, applyDeltas, new position written
//                  in place (a thread reads and writes only its own particles here, so the write needs no barrier of its own).
// Same operations per particle in the same order as fs_k_fused_step (springs, its contacts in list order, shapes, applyDeltas).
// The overflow queue: a particle with contact candidates that found no room in the contact set (which takes the 1024 longest
// lists; what is left over has one candidate, in a crowded episode two) queues in the LDS the hash tables leave idle during the
// iterations, and the lanes of waves 1..15 evaluate its contacts 64 to a wavefront in the shadow of wave 0, which holds the
// longest lists of the set and is what the contact phase waits for anyway.  What a queue lane needs to know about its entries
// -- particle | first candidate << 12 | (candidates - 1) << 28 -- is written once per substep at allotment and kept in two
// registers of the lane.  A particle with candidates that gets neither (set and queue full, or a list longer than 16 outside
// the set: FG_SLOT_INLINE) evaluates its contacts in the spring phase, where every position still is the old iterate.
#ifndef FG_SINGLES
#define FG_SINGLES 1
#endif
#define FG_SINGLES_LANES (FS_FUSED_THREADS - 64)                                  // waves 1..15, two rounds at most
#define FG_SINGLES_ROOM ((FS_FUSED_CUR_BYTES + FS_FUSED_MAX_PARTICLES * 2) / 16)  // 1536 entries of 16 B
#define FG_SINGLES_CAP (FG_SINGLES_ROOM < 2 * FG_SINGLES_LANES ? FG_SINGLES_ROOM : 2 * FG_SINGLES_LANES)
#define FG_SLOT_NONE 0xffffu                   // 16-bit slot values: no candidates -> sums stay in registers
#define FG_SLOT_INLINE 0xfffeu                 // candidates, but no room in set or queue -> contacts in the spring phase
static_assert(FS_FUSED_CSET_CAP + FG_SINGLES_CAP <= FG_SLOT_INLINE, "slot values below the reserved ones");

// Particle k (0..3) of thread t = 64 w + lane in the Jacobi iterations and the contact set: trip k >> 1 owns the two
// ADJACENT rows P = 2 w + 32 (k >> 1) and Q = P + 1 (k & 1), so every spring between P and Q stays inside the wavefront.
#define FG_ROW(w, k) (2 * (w) + 32 * ((k) >> 1) + ((k) & 1))

// One canonical slot for the pair (P = row r, Q = row r + 1) of the thread: three ds_read2st64_b32, each returning the
// P and Q halves of one coordinate in a register pair.  `a` = LDS byte address of (row r - 2, column + dx) in the x
// plane; rows and planes are immediates (offsets count 64 floats = one row; the x | y | z planes are 64 rows apart).
// Written as inline assembly because the compiler's load merger, given plain loads, pairs whatever two loads it meets
// first (neighbouring columns, the rows of two different slots) and then shuffles the halves back with v_mov.  The
// compiler does not know these are LDS reads, so FG_WAIT -- through which the loaded registers are routed, making every
// consumer depend on it -- carries the s_waitcnt: lgkmcnt(N) with N = number of reads issued AFTER the ones awaited
// (LDS returns in order, so any further outstanding operation only makes the wait longer, never shorter).
template <int DZ>
__device__ __forceinline__ void fg_load_slot(unsigned a, fs_f2 &x0, fs_f2 &x1, fs_f2 &x2) {
    asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(x0) : "v"(a), "n"(DZ + 2), "n"(DZ + 3) : "memory");
    asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(x1) : "v"(a), "n"(DZ + 2 + 64), "n"(DZ + 3 + 64) : "memory");
    asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(x2) : "v"(a), "n"(DZ + 2 + 128), "n"(DZ + 3 + 128) : "memory");
}
// (value of row r, value of row r + 1) of a row-indexed [.][64] table, r even: one ds_read_b64.  `a` = address of entry r of
// the first table; OFF = byte offset of the table wanted (a 16-bit immediate, so one address serves every row table).
template <int OFF>
__device__ __forceinline__ fs_f2 fg_load_rows(unsigned a) {
    static_assert(OFF >= 0 && OFF < 65536 && OFF % 8 == 0, "ds_read_b64 offset");
    fs_f2 r;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(a), "n"(OFF) : "memory");
    return r;
}
// (row R0, row R1) of a column-indexed [.][64] table at the lane's column: one ds_read2st64_b32, rows as immediates
template <int R0, int R1>
__device__ __forceinline__ fs_f2 fg_load_cols(unsigned a) {
    static_assert(R0 >= 0 && R0 < 256 && R1 >= 0 && R1 < 256, "ds_read2st64_b32 offsets");
    fs_f2 r;
    asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(r) : "v"(a), "n"(R0), "n"(R1) : "memory");
    return r;
}
#define FG_WAIT(N, A0, A1, A2) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(A0), "+v"(A1), "+v"(A2))

// fs_spring_fast, split in two.  fg_scale: the scale of spring (i, j), kh * (C / length) with kh = stiffness / 2 (or 0 for
// a slot outside the grid: the scale then is +-0 and leaves the accumulators as they are), and its squared length.
// fg_accum: the particle's own difference and the three accumulations.  Both endpoints of a spring get the SAME scale
// bits: xj - xi is exactly -(xi - xj), the squared length of a negated vector is the same, and the host verifies that
// the rest length and the stiffness of a slot equal those of the reverse slot at the partner (build_grid64) -- so a
// scale computed at one endpoint can be handed to the other.
// (A packed version on v_pk_add/mul/fma_f32 -- the (P, Q) register pairs are exactly its operand shape -- was built and
// measured: bit-identical, 14 % SLOWER.  On this part a packed fp32 instruction occupies the VALU for as long as two
// scalar ones, so packing buys no throughput and lengthens the dependent chains; EXPERIMENTS.md "packed fp32".)
// The root is v_rsq_f32 WITHOUT fs_rsqrt's max(l2, FLT_MIN) in front: for a squared length of at least FLT_MIN the clamp returns
// its operand, so the bits are the same and the v_max_f32 per spring (17 per trip) is gone; a pair that meets a smaller one
// -- 0 for coincident particles, a denormal for particles ~1e-19 apart -- is sent down the exact path by the running minimum,
// which tests `< FG_MIN_L2` where it used to test `== 0`, and fs_spring there clamps as ever.
#define FG_MIN_L2 1.17549435e-38f
__device__ __forceinline__ float fg_scale(float xi0, float xi1, float xi2, float xj0, float xj1, float xj2, float L, float k,
                                          float &l2) {
    const float ex = xi0 - xj0, ey = xi1 - xj1, ez = xi2 - xj2;
    l2 = fs_dot3(ex, ey, ez, ex, ey, ez);
    const float inv = __builtin_amdgcn_rsqf(l2);  // = fs_rsqrt(l2) for every l2 >= FG_MIN_L2
    const float len = l2 * inv;
    const float C = len - L;
    return k * (C * inv);
}
__device__ __forceinline__ void fg_accum(float &d0, float &d1, float &d2, float xi0, float xi1, float xi2, float xj0, float xj1,
                                         float xj2, float sc) {
    const float ex = xi0 - xj0, ey = xi1 - xj1, ez = xi2 - xj2;
    d0 = FS_FMA(-ex, sc, d0);
    d1 = FS_FMA(-ey, sc, d1);
    d2 = FS_FMA(-ez, sc, d2);
}
// the value of lane - 1 / lane + 1 of the wavefront (+0 in lane 0 / lane 63): one v_mov_b32_dpp wave_shr:1 / wave_shl:1
// with bound_ctrl
__device__ __forceinline__ float fg_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float fg_from_right(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

// fs_apply with the quotient relaxationFactor / count from the LDS table (the same IEEE division, done once per launch)
__device__ __forceinline__ void fg_apply(const FsAcc &a, float relax, const float *rcnt, float &x0, float &x1, float &x2) {
    if (a.cnt > 0) {
        const float sc = a.cnt < 128 ? rcnt[a.cnt] : relax / (float)a.cnt;
        x0 = FS_FMA(a.d0, sc, x0); x1 = FS_FMA(a.d1, sc, x1); x2 = FS_FMA(a.d2, sc, x2);
    }
}

__global__ __launch_bounds__(FS_FUSED_THREADS) void fs_k_fused_grid64(const FsEnvDev *__restrict__ envs,
                                                                      const FsShapesDev *__restrict__ shapes, const int *ids,
                                                                      int n_steps) {
    static_assert(FS_FUSED_THREADS == 1024 && FS_FUSED_PPT == 4, "grid-64 kernel: 16 waves x 4 rows");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *Xx = (float *)(smem + FG_OFF_XX);
    float *Xy = Xx + FS_FUSED_MAX_PARTICLES, *Xz = Xy + FS_FUSED_MAX_PARTICLES, *Xw = Xz + FS_FUSED_MAX_PARTICLES;
    float *X0x = (float *)(smem + FG_OFF_X0);
    float *X0y = X0x + FS_FUSED_MAX_PARTICLES;
    float *X0z = X0y + FS_FUSED_MAX_PARTICLES;
    unsigned short *cursor = (unsigned short *)(smem + FG_OFF_CUR);
    unsigned short *items = (unsigned short *)(smem + FG_OFF_ITEMS);
    int *wave_tot = (int *)(smem + FG_OFF_SCAN);
    float *rowL = (float *)(smem + FG_OFF_ROWL);

#ifdef FS_BLOCK_CLOCKS  // developer build: how long every workgroup runs (scripts/block_clocks.py)
    const unsigned long long tc_start = __builtin_amdgcn_s_memtime(), tr_start = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef FS_TIMING  // developer build: per-section shader-clock totals of block 0's waves, printed at the end (FS_TS).
                  // Block 0 of the bench is a light episode: it is done before the printing of others disturbs anything,
                  // but its numbers are not those of the episodes a launch waits for (scripts/block_clocks.py).
    unsigned long long ts_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long ts_last = __builtin_amdgcn_s_memtime();
#endif
    const int e = ids[blockIdx.x];
    if (e < 0) return;  // slot retired by a device-side loop (fs_wait_until_stable)
    const FsEnvDev &E = envs[e];
    const FsShapesDev &sh = shapes[e];
    const FsFusedConsts c = fs_fused_consts(E, sh);
    const int n = c.n;
    const unsigned un = (unsigned)n;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int dimz = n >> 6;

    FsVec4 *const g_pos = E.pos;
    const FsVec4 *const g_rest = E.rest;
    const fs_gci g_phase = (fs_gci)E.phase;
    const fs_gi g_nlist = (fs_gi)E.nlist, g_ncount = (fs_gi)E.ncount;
    const fs_gci g_ell_j = (fs_gci)E.ell_j;
    const fs_gcf g_ell_len = (fs_gcf)E.ell_len, g_ell_k = (fs_gcf)E.ell_k;
    const fs_gcf g_L = (fs_gcf)E.g64_L;
    const int max_deg = E.max_deg;
    const fs_gcu g_near = (fs_gcu)E.restnear_w;

    // one phase for the whole cloth? (see fs_k_fused_step)
    int find_mode = 0;
    {
        const int ph0 = g_phase[0];
        int differs = 0;
        for (int i = t; i < n; i += FS_FUSED_THREADS) differs |= (g_phase[i] != ph0);
        if (t == 0) wave_tot[0] = 0;
        __syncthreads();
        if (differs) atomicOr(&wave_tot[0], 1);
        __syncthreads();
        const int mixed = wave_tot[0];
        __syncthreads();
        if (!mixed) {
            if (!(ph0 & FS_PHASE_SELF_COLLIDE)) find_mode = 3;
            else if (!(ph0 & FS_PHASE_SELF_COLLIDE_FILTER)) find_mode = 2;
            else if (E.restnear_ok == 2 && FS_STENCIL_FILTER) find_mode = 4;
            else if (E.restnear_ok) find_mode = 1;
        }
    }
    // Everything a gather can touch holds finite numbers from here on: pad, the four planes (rows past the cloth stay 0).
    for (int q = t; q < FG_OFF_X0 / 4; q += FS_FUSED_THREADS) ((float *)smem)[q] = 0.0f;
    __syncthreads();
    for (int i = t; i < n; i += FS_FUSED_THREADS) {
        const FsVec4 p = fs_ld4(g_pos, i);
        Xx[i] = p.x; Xy[i] = p.y; Xz[i] = p.z; Xw[i] = p.w;
        X0x[i] = p.x; X0y[i] = p.y; X0z[i] = p.z;
    }
    // rest lengths.  z-direction slots 8..11 per row -> LDS (taken from column 2, valid for every in-grid slot)
    if (t < 256) {
        const int r = t & 63, s = 8 + (t >> 6);
        rowL[t] = r < dimz ? g_L[(unsigned)s * un + (unsigned)(r * 64 + 2)] : 0.0f;
    }
    // x-direction slots 0, 1 per column (taken from row 2; 0 where the column lacks the slot) -> LDS.  Slots 4, 5 take the
    // scales of the s0 / s1 of the lanes to their right and need no rest length.
    constexpr int XS_DX[4] = {-1, -2, +1, +2};
    constexpr int SH_DX[4] = {+1, -1, -1, +1}, SH_DZ[4] = {-1, -1, +1, +1};
    constexpr int ZS_DZ[4] = {-1, -2, +1, +2};
    float *colL = (float *)(smem + FG_OFF_COLL);
    if (t < 128) {
        const int col = t & 63, q = t >> 6;
        const int dxq = q == 0 ? -1 : -2;  // slot q = 0, 1
        colL[t] = (unsigned)(col + dxq) < 64u ? g_L[(unsigned)q * un + (unsigned)(2 * 64 + col)] : 0.0f;
    }
    // applyDeltas' relaxationFactor / count for every count a particle can reach (12 springs + 96 contacts + planes +
    // spheres < 128): the correctly rounded quotient, computed once instead of once per particle and iteration
    float *rcnt = (float *)(smem + FG_OFF_RCNT);
    if (t < 128) rcnt[t] = t > 0 ? c.relax / (float)t : 0.0f;
    // stiffness / 2 of the slots whose row or column has to have them, with +0 where it has not: shear slots 2, 3, 6, 7 per
    // column, z-direction slots 8..11 per row.  (A shear slot also needs its row: the trips at the cloth's first and last
    // rows read the +0 of the pad instead.)  Slots 4, 5 and P's 6, 7, 10 take shared scales and need no stiffness.
    if (t < 256) {
        const int c64 = t & 63, q = t >> 6;
        const int sdx = (q == 0 || q == 3) ? +1 : -1, sslot = q < 2 ? 2 + q : 4 + q;  // = SH_DX[q], SH_SLOT[q]
        const int zdz = q < 2 ? -1 - q : q - 1;                                       // = ZS_DZ[q]
        ((float *)(smem + FG_OFF_KS))[t] = (unsigned)(c64 + sdx) < 64u ? E.g64_kh[sslot] : 0.0f;
        ((float *)(smem + FG_OFF_KZ))[t] = (c64 < dimz && (unsigned)(c64 + zdz) < (unsigned)dimz) ? E.g64_kh[8 + q] : 0.0f;
    }
    // stiffness / 2 of the x-direction slots 0, 1 (wave-uniform)
    const float kh0 = E.g64_kh[0], kh1 = E.g64_kh[1];
    // number of in-grid slots of each of the thread's particles (8 bits per particle)
    unsigned nvalid = 0u;
#pragma unroll
    for (int k = 0; k < FS_FUSED_PPT; ++k) {
        const int row = FG_ROW(w, k);
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cnt += ((unsigned)(lane + XS_DX[q]) < 64u) ? 1 : 0;
            cnt += ((unsigned)(lane + SH_DX[q]) < 64u && (unsigned)(row + SH_DZ[q]) < (unsigned)dimz) ? 1 : 0;
            cnt += ((unsigned)(row + ZS_DZ[q]) < (unsigned)dimz) ? 1 : 0;
        }
        nvalid |= (unsigned)cnt << (8 * k);
    }
    __syncthreads();
    // bit k: every lane's particle k of this wave is dynamic and all its in-grid neighbours carry its own inverse mass
    // (constant for the launch) -> the packed spring form applies
    unsigned fastmask = 0u;
    {
        constexpr int cdx[FS_G64_SLOTS] = FS_G64_DX_LIST, cdz[FS_G64_SLOTS] = FS_G64_DZ_LIST;
#pragma unroll
        for (int k = 0; k < FS_FUSED_PPT; ++k) {
            const int row = FG_ROW(w, k), i = row * 64 + lane;
            bool differs = false;
            if (i < n) {
                const float wi = Xw[i];
                differs = !(wi > 0.0f);
#pragma unroll
                for (int q = 0; q < FS_G64_SLOTS; ++q) {
                    const bool in = (unsigned)(lane + cdx[q]) < 64u && (unsigned)(row + cdz[q]) < (unsigned)dimz;
                    if (in) differs |= Xw[i + cdz[q] * 64 + cdx[q]] != wi;
                }
            }
            if (i < n && __builtin_amdgcn_ballot_w64(differs) == 0ull) fastmask |= 1u << k;
        }
        fastmask = (unsigned)__builtin_amdgcn_readfirstlane((int)fastmask);  // wave-uniform: a scalar register, tested with scalar instructions
    }

    // What a substep starts from, for the thread's particles t + k * 1024: position (w = inverse mass) and velocity.  Loaded
    // here for the first substep of the launch; every later substep -- the first of the next frame like any other -- takes
    // them from the finalize of the substep before, which the same thread runs on the same particles: finalize and predict
    // are ONE pass over registers, the velocity is loaded once per substep (four loads in flight, one wait), and X0 is not
    // written to LDS only to be read back.
    FsVec4 sx[FS_FUSED_PPT], sv[FS_FUSED_PPT];
#pragma unroll
    for (int k = 0; k < FS_FUSED_PPT; ++k) {
        const int i = t + k * FS_FUSED_THREADS;
        sx[k] = FsVec4{0.0f, 0.0f, 0.0f, 0.0f};
        sv[k] = FsVec4{0.0f, 0.0f, 0.0f, 0.0f};
        if (i < n) {
            sv[k] = fs_ld4o(E.vel, (unsigned)i);
            sx[k] = FsVec4{X0x[i], X0y[i], X0z[i], Xw[i]};
        }
    }

    FS_TS(0)
#pragma unroll 1
    for (int frame = 0; frame < n_steps; ++frame) {
#pragma unroll 1
        for (int sub = 0; sub < c.substeps; ++sub) {
            // ---- predict from (sx, sv); build the spatial hash (XS = bucket-ordered copy in the X0 region)
            FsVec4 xp[FS_FUSED_PPT];
            {
                // (the lane's index is formed here, in the pass: an address hoisted out of the frame loop is one more register
                // the iterations spill -- as for aLane in the spring trip -- and its reload here would wait for the velocity
                // stores of the finalize in front)
                unsigned tl = (unsigned)t;
                asm volatile("" : "+v"(tl));
                for (unsigned q = tl; q < FS_FUSED_BUCKETS / 2; q += FS_FUSED_THREADS) ((unsigned *)cursor)[q] = 0u;
                FsFusedConsts cf = c;  // the pass's constants, fetched together (see finalize)
                asm volatile("" : "+v"(cf.h), "+v"(cf.g0), "+v"(cf.g1), "+v"(cf.g2), "+v"(cf.damping));
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    xp[k] = FsVec4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (i < un) xp[k] = fs_fused_predict(cf, sx[k], sv[k]);
                }
                // X0 is parked in global memory across the search (its LDS holds XS); w rides along.  The four stores close
                // the pass: nothing behind them waits for their acknowledgement but the barrier.
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    if (i < un) fs_st4o(E.x0, i, sx[k]);
                }
            }
            FS_TS(12)
            __syncthreads();
            // find mode 4: the append counts of the half-stencil search, in the z plane (every plane is dead until the restore
            // below: the predicted positions sit in their owners' registers, and the barriers of the hash build follow)
            const fs_lu fill = (fs_lu)(smem + FG_OFF_XX + 2 * FG_PLANE);
            // ... and the heads of the lists (appends 0..3 of every particle, fs_pair_append): rows 0, 1 in the w plane, which
            // the restore rewrites from the parked X0 word, rows 2, 3 in the contact set's accumulators, which the first spring
            // phase of the substep rewrites.  Written between the hash build and the search's first barrier, read by the sort
            // pass, dead at the second barrier -- behind which the over-the-cap search lays its queues over all four planes.
            const fs_lus heads = (fs_lus)(smem + FG_OFF_XX + 3 * FG_PLANE);
            static_assert(FG_OFF_CACC - (FG_OFF_XX + 3 * FG_PLANE) == FS_PAIR_HEADS_HI * 2, "heads: rows 2, 3 start at the set's accumulators");
            static_assert(FS_FUSED_CSET_CAP * 16 >= 2 * FS_FUSED_MAX_PARTICLES * 2 && FG_PLANE >= 2 * FS_FUSED_MAX_PARTICLES * 2,
                          "heads: two rows of 16-bit ids per region");
            if (find_mode == 4) {
                unsigned tl = (unsigned)t;
                asm volatile("" : "+v"(tl));
                for (unsigned q = tl; q < FS_FUSED_MAX_PARTICLES; q += FS_FUSED_THREADS) fill[q] = 0u;
            }
            // The predicted positions are not kept across the search: XS is xp permuted and stays valid until the restore, so
            // the thread keeps where its four particles went (16 bits each) and reads them back from there.
            unsigned xslot[2];
            {
                int slot_of[FS_FUSED_PPT] = {0, 0, 0, 0};
                fs_fused_build_grid(c, xp, cursor, items, wave_tot, X0x, X0y, X0z, slot_of);
                xslot[0] = (unsigned)slot_of[0] | ((unsigned)slot_of[1] << 16);
                xslot[1] = (unsigned)slot_of[2] | ((unsigned)slot_of[3] << 16);
            }
            FS_TS(1)
            const FsFindConsts fc = {n, c.ncap, c.rad2, c.inv_rad, find_mode, E.gp_dimx, E.gp_magic};
            if (find_mode == 4) {  // grid cloth: every pair found once, by its owner (fs_pair_search.h)
                int *const any_over = wave_tot;  // (the hash build's scratch: idle)
                if (t == 0) *any_over = 0;
                int sb0 = 0, sb1 = 0, sb2 = 0, sb3 = 0;  // shape candidates of the thread's particles, kept across the barrier
#pragma unroll 1
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const int qs = t + k * FS_FUSED_THREADS;
                    if (qs >= n) break;
                    const int i = items[qs];
                    const FsVec4 xi = FsVec4{X0x[qs], X0y[qs], X0z[qs], 0.0f};  // = XS[qs], the predicted position of i
                    const int shape_bits = (int)(fs_shape_candidates(E.p, sh, sub, xi.x, xi.y, xi.z) << FS_SHAPE_MASK_SHIFT);
                    if (k == 0) sb0 = shape_bits; else if (k == 1) sb1 = shape_bits; else if (k == 2) sb2 = shape_bits; else sb3 = shape_bits;
                    fs_pair_find_neighbors(fc, i, qs, xi, (fs_lcus)cursor, (fs_lcus)items, g_nlist, (fs_lus)(smem + FG_OFF_XX) + t,
                                           (fs_lcf)X0x, fill, heads);
                }
                FS_TS(2)
                __syncthreads();  // every append is made
                FS_TS(3)
                unsigned overmask = 0u;
#pragma unroll 1
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const int qs = t + k * FS_FUSED_THREADS;
                    if (qs >= n) break;
                    const int i = items[qs];
                    const int cnt = (int)fill[i];
                    const int shape_bits = k == 0 ? sb0 : k == 1 ? sb1 : k == 2 ? sb2 : sb3;
                    if (cnt > c.ncap) {  // the appends kept the first ncap, not the smallest: searched again below
                        overmask |= 1u << k;
                        continue;
                    }
                    fs_pair_sort_column(n, i, cnt, g_nlist, (fs_lcus)heads);
                    g_ncount[i] = cnt | shape_bits;
                }
                if (overmask) atomicOr(any_over, 1);
                __syncthreads();  // every thread has read its counts and its heads; XS and the hash are still valid
                if (*any_over) {  // (uniform) a pile: the one-sided search keeps the smallest ids; its queue covers all four planes
                    FsNearWords none;
#pragma unroll
                    for (int q = 0; q < 8; ++q) none.w[q] = 0xffffffffu;
#pragma unroll 1
                    for (int k = 0; k < FS_FUSED_PPT; ++k) {
                        if (!((overmask >> k) & 1u)) continue;
                        const int qs = t + k * FS_FUSED_THREADS;
                        const int i = items[qs];
                        const FsVec4 xi = FsVec4{X0x[qs], X0y[qs], X0z[qs], 0.0f};
                        const int shape_bits = k == 0 ? sb0 : k == 1 ? sb1 : k == 2 ? sb2 : sb3;
                        g_ncount[i] = fs_fused_find_neighbors<true>(fc, i, xi, (fs_lcus)cursor, (fs_lcus)items, g_phase, g_rest, g_nlist,
                                                                    none, (fs_lus)(smem + FG_OFF_XX) + t, (fs_lcf)X0x) | shape_bits;
                    }
                    __syncthreads();  // every wave is done with XS, the hash and the queues
                }
                FS_TS(15)
            } else {
#pragma unroll 1
                for (int qs = t; qs < n; qs += FS_FUSED_THREADS) {
                    const int i = items[qs];
                    const FsVec4 xi = FsVec4{X0x[qs], X0y[qs], X0z[qs], 0.0f};  // = XS[qs], the predicted position of i
                    // collideShapes rides along: the particle's shape candidates go into the upper bits of its count word
                    const int shape_bits = (int)(fs_shape_candidates(E.p, sh, sub, xi.x, xi.y, xi.z) << FS_SHAPE_MASK_SHIFT);
                    FsNearWords near;
#pragma unroll
                    for (int q = 0; q < 8; ++q) near.w[q] = find_mode == 1 ? g_near[(unsigned)q * un + (unsigned)i] : 0xffffffffu;
                    g_ncount[i] = (find_mode == 3 ? 0
                                                  : fs_fused_find_neighbors<false>(fc, i, xi, (fs_lcus)cursor, (fs_lcus)items, g_phase,
                                                                                   g_rest, g_nlist, near,
                                                                                   (fs_lus)(smem + FG_OFF_XX) + t, (fs_lcf)X0x)) |
                                  shape_bits;
                }
                FS_TS(2)
                __syncthreads();  // every wave is done with XS, the hash and the queues (which covered the planes)
                FS_TS(3)
            }
            // ---- restore.  Every wave is past its last read of XS, the hash and the queues (the barriers above), the count
            // words are written.  One batch of loads -- the parked X0 of the thread's particles and the count words of its
            // iteration rows -- travels while the predicted positions go from XS to the planes; X0 itself, whose region XS
            // occupies, is written behind the next barrier, when every thread has read its part of XS.
            FsVec4 p0r[FS_FUSED_PPT];
            int cword[FS_FUSED_PPT];
            {
                unsigned tl = (unsigned)t;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    p0r[k] = fs_ld4o(E.x0, i < un ? i : 0u);
                }
                const unsigned wl = tl >> 6, ll = tl & 63u;
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = (unsigned)FG_ROW(wl, k) * 64u + ll;
                    cword[k] = fs_ldo((const int *)E.ncount, i < un ? i : 0u);
                }
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    const unsigned s = (xslot[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                    const float x = X0x[s], y = X0y[s], z = X0z[s];  // = XS[s], the predicted position of i
                    if (i < un) {
                        Xx[i] = x; Xy[i] = y; Xz[i] = z; Xw[i] = p0r[k].w;
                    } else {
                        Xx[i] = 0.0f; Xy[i] = 0.0f; Xz[i] = 0.0f; Xw[i] = 0.0f;  // rows past the cloth: finite again
                    }
                }
            }

            FS_TS(13)
            // ---- contact set (see fs_k_fused_step)
            unsigned short *cset = (unsigned short *)(smem + FG_OFF_CSET);
            FsVec4 *cacc = (FsVec4 *)(smem + FG_OFF_CACC);
            int *chist = (int *)(smem + FG_OFF_CHIST);
            if (t < 128) chist[t] = 0;
            int *nsingles = (int *)(smem + FG_OFF_SCAN);  // (the hash build's scratch: idle)
            if (t == 0) *nsingles = 0;
            __syncthreads();
            {
                unsigned tl = (unsigned)t;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    if (i < un) { X0x[i] = p0r[k].x; X0y[i] = p0r[k].y; X0z[i] = p0r[k].z; }
                }
            }
            // (wave and lane of the two passes below, formed here: see predict)
            unsigned tq = (unsigned)t;
            asm volatile("" : "+v"(tq));
            const int wq = (int)(tq >> 6), lq = (int)(tq & 63u);
            int ccls[FS_FUSED_PPT];
#pragma unroll
            for (int k = 0; k < FS_FUSED_PPT; ++k) {
                const int i = FG_ROW(wq, k) * 64 + lq;
                int cc = 0;
                if (i < n && Xw[i] > 0.0f) cc = cword[k] & FS_NCOUNT_MASK;
                ccls[k] = cc > 96 ? 96 : cc;
                if (ccls[k] > 0) atomicAdd(&chist[ccls[k]], 1);
            }
            __syncthreads();
            fs_fused_count_offsets(chist, t);
            __syncthreads();
            FsVec4 *squeue = cacc + FS_FUSED_CSET_CAP;
            unsigned slotw[2] = {~0u, ~0u};  // the 16-bit slot values of the thread's particles, one word per trip: P | Q << 16
#pragma unroll
            for (int k = 0; k < FS_FUSED_PPT; ++k) {
                if (ccls[k] > 0) {
                    const int i = FG_ROW(wq, k) * 64 + lq;
                    unsigned slot = FG_SLOT_INLINE;
                    const int pos = atomicAdd(&chist[ccls[k]], 1);
                    if (pos < FS_FUSED_CSET_CAP) {
                        cset[pos] = (unsigned short)i;
                        slot = (unsigned)pos;
                    }
#if FG_SINGLES
                    else if (ccls[k] <= 16) {  // slot value CAP + place in the overflow queue
                        const int sp = atomicAdd(nsingles, 1);
                        if (sp < FG_SINGLES_CAP) {
                            slot = (unsigned)(FS_FUSED_CSET_CAP + sp);
                            // what the queue lane has to know, read by it once below (the iterations overwrite the entry)
                            squeue[sp].w = __int_as_float(i | (fs_ldo((const int *)E.nlist, (unsigned)i) << 12) | ((ccls[k] - 1) << 28));
                        }
                    }
#endif
                    slotw[k >> 1] = (slotw[k >> 1] & ~(0xffffu << (16 * (k & 1)))) | (slot << (16 * (k & 1)));
                }
            }
            FS_TS(14)
            __syncthreads();
            const int csize = chist[0] < FS_FUSED_CSET_CAP ? chist[0] : FS_FUSED_CSET_CAP;
            const int n_singles = *nsingles < FG_SINGLES_CAP ? *nsingles : FG_SINGLES_CAP;
            const int i2 = t < csize ? (int)cset[t] : -1;
            int cnt2 = 0, cj2[FS_FUSED_PREFETCH_CAND];
#pragma unroll
            for (int q = 0; q < FS_FUSED_PREFETCH_CAND; ++q) cj2[q] = 0;
            if (i2 >= 0) {
                cnt2 = g_ncount[i2] & FS_NCOUNT_MASK;
#pragma unroll
                for (int q = 0; q < FS_FUSED_PREFETCH_CAND; ++q) cj2[q] = g_nlist[(unsigned)q * un + (unsigned)i2];
            }
            // the (at most two) queue entries of this lane
            static_assert(FG_SINGLES_CAP <= 2 * FG_SINGLES_LANES, "two queue entries per lane");
            unsigned qw0 = 0u, qw1 = 0u;
#if FG_SINGLES
            if (t >= 64 && t - 64 < n_singles) qw0 = (unsigned)__float_as_int(squeue[t - 64].w);
            if (t >= 64 && t - 64 + FG_SINGLES_LANES < n_singles) qw1 = (unsigned)__float_as_int(squeue[t - 64 + FG_SINGLES_LANES].w);
            __syncthreads();  // every lane has its words: the spring phase may write the entries
#endif

            FS_TS(4)
            // ---- Jacobi iterations
#pragma unroll 1
            for (int it = 0; it < c.iters; ++it) {
                // spring sums of the thread's particles (those without a slot are finished from here) and their counts, 8 bits each
                unsigned cpack = 0u;
                // the sums of one trip's P and Q, statically named: `rnew` is the trip that parked last, `rold` the one before
                float rold[2][3], rnew[2][3];
#pragma unroll
                for (int q = 0; q < 6; ++q) { rold[q / 3][q % 3] = 0.0f; rnew[q / 3][q % 3] = 0.0f; }
#ifdef FG_UNROLL_PAIRS
#pragma unroll
#else
#pragma unroll 1
#endif
                for (int pr = 0; pr < 2; ++pr) {
                    const int rowP = FG_ROW(w, 2 * pr);            // wave-uniform; row Q = rowP + 1
                    const int iP_raw = rowP * 64 + lane, iQ_raw = iP_raw + 64;
                    const bool haveP = rowP < dimz, haveQ = rowP + 1 < dimz;
                    const int iP = haveP ? iP_raw : 0, iQ = haveQ ? iQ_raw : 0;
                    const bool fast = haveQ && ((fastmask >> (2 * pr)) & 3u) == 3u;
                    // own positions of the pair
                    const fs_f2 xi0 = fs_f2{Xx[iP], Xx[iQ]}, xi1 = fs_f2{Xy[iP], Xy[iQ]}, xi2 = fs_f2{Xz[iP], Xz[iQ]};
                    const fs_f2 wi = fs_f2{Xw[iP], Xw[iQ]};
                    FsAcc aP, aQ;  // set by the fast block, or from zero by the exact path
                    bool exact = !fast;
                    if (fast) {
                        // LDS byte address of (row P - 2, column + dx) in the x plane for dx = -2..2
                        // (the lane's part is formed here, in the trip: hoisted out of the loops it would be one more register held
                        // across the whole frame)
                        unsigned aLane = (unsigned)(lane * 4);
                        asm volatile("" : "+v"(aLane));
                        const unsigned am2 = (unsigned)(FG_OFF_XX + ((rowP - 2) * 64 - 2) * 4) + aLane;
                        const unsigned am1 = am2 + 4u, a00 = am2 + 8u, ap1 = am2 + 12u, ap2 = am2 + 16u;
                        // shear rest lengths the pair evaluates itself: P's slots 2, 3 and Q's 2, 3, 6, 7 (per particle, from
                        // L2, well ahead of their use; P's slots 6 and 7 take Q's scales)
                        constexpr int SH_SLOT[4] = {2, 3, 6, 7};
                        float sLP[2], sLQ[4];
#pragma unroll
                        for (int q = 0; q < 2; ++q) sLP[q] = g_L[(unsigned)SH_SLOT[q] * un + (unsigned)iP];
#pragma unroll
                        for (int q = 0; q < 4; ++q) sLQ[q] = g_L[(unsigned)SH_SLOT[q] * un + (unsigned)iQ];
                        // x-direction rest lengths of slots 0, 1 of this column: LDS table, issued first so that it is older than
                        // every gather below (slots 4, 5 take shared scales)
                        // (one address per kind of table: the column tables KS | COLL at the lane, the row tables ROWL | KZ at row P)
                        const unsigned aRow = (unsigned)(FG_OFF_ROWL + rowP * 4), aCol = (unsigned)FG_OFF_KS + aLane;
                        constexpr int CL_ROW = (FG_OFF_COLL - FG_OFF_KS) / 256;
                        fs_f2 cL = fg_load_cols<CL_ROW, CL_ROW + 1>(aCol);
                        // stiffness of the shear slots the pair evaluates, from the column table (0 = column + dx outside the
                        // grid): P's s2, s3 exist from row 1 on, Q's s2, s3 always (row P is there), Q's s6, s7 while row
                        // P + 2 is inside.  A trip whose row lacks them reads rows 0, 1 / 2, 3 of the pad -- +0 -- through the
                        // same immediates.
                        const unsigned aKP = rowP >= 1 ? aCol : aLane;
                        const unsigned aKQ = rowP + 2 < dimz ? aCol : aLane;
                        fs_f2 kP23 = fg_load_cols<0, 1>(aKP);
                        fs_f2 kQ23 = fg_load_cols<0, 1>(aCol);
                        // stiffness of the x-direction slots 0, 1 (loop-invariant registers)
#define FG_KX(q) ((unsigned)(lane + XS_DX[q]) < 64u ? (q == 0 ? kh0 : kh1) : 0.0f)
                        // accumulators of P and Q (from +0), running minimum of the squared lengths of each (all evaluated
                        // slots: one outside the grid reads unrelated finite data, which at worst sends a pair down the exact
                        // path for nothing)
                        float dP0 = 0.0f, dP1 = 0.0f, dP2 = 0.0f, dQ0 = 0.0f, dQ1 = 0.0f, dQ2 = 0.0f, mP = 1.0f, mQ = 1.0f;
                        fs_f2 u0, u1, u2, v0, v1, v2;
                        float l2a, l2b, l2c, l2d;
                        // ---- canonical order s0..s11 for both particles; the gathers of slot s + 1 are issued before the
                        // arithmetic of slot s.  A spring inside the wavefront is evaluated by the endpoint whose slot comes
                        // FIRST in this order -- s0, s1 of P and Q, and Q's s2, s3, s8 -- and its scale is kept for the partner's
                        // slot further down (lane c-1's s4 / c-2's s5 in the same row; P's s6 at c+1, s7 at c-1, s10 at c): no
                        // position is gathered twice and no difference is taken twice.
                        fg_load_slot<0>(am1, u0, u1, u2);                                   // s0 (-1, 0)
                        fg_load_slot<0>(am2, v0, v1, v2);                                   // s1 (-2, 0)
                        asm volatile("s_waitcnt lgkmcnt(3)"
                                     : "+v"(cL), "+v"(kP23), "+v"(kQ23), "+v"(u0), "+v"(u1), "+v"(u2));
                        const float scP0 = fg_scale(xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, cL.x, FG_KX(0), l2a);
                        const float scQ0 = fg_scale(xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, cL.x, FG_KX(0), l2b);
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, scP0);
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, scQ0);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<-1>(ap1, u0, u1, u2);                                  // s2 (+1, -1)
                        FG_WAIT(3, v0, v1, v2);
                        const float scP1 = fg_scale(xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, cL.y, FG_KX(1), l2c);
                        const float scQ1 = fg_scale(xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, cL.y, FG_KX(1), l2d);
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, scP1);
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, scQ1);
                        mP = fminf(fminf(mP, l2a), l2c);
                        mQ = fminf(fminf(mQ, l2b), l2d);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<-1>(am1, v0, v1, v2);                                  // s3 (-1, -1)
                        FG_WAIT(3, u0, u1, u2);
                        const float scQ2 = fg_scale(xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, sLQ[0], kQ23.x, l2b);
                        {
                            const float sc = fg_scale(xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, sLP[0], kP23.x, l2a);
                            fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, sc);
                        }
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, scQ2);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<0>(ap1, u0, u1, u2);                                   // s4 (+1, 0)
                        FG_WAIT(3, v0, v1, v2);
                        const float scQ3 = fg_scale(xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, sLQ[1], kQ23.y, l2d);
                        {
                            const float sc = fg_scale(xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, sLP[1], kP23.y, l2c);
                            fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, sc);
                        }
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, scQ3);
                        mP = fminf(fminf(mP, l2a), l2c);
                        mQ = fminf(fminf(mQ, l2b), l2d);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<0>(ap2, v0, v1, v2);                                   // s5 (+2, 0)
                        FG_WAIT(3, u0, u1, u2);
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, fg_from_right(scP0));
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, fg_from_right(scQ0));
                        __builtin_amdgcn_sched_barrier(0);
                        fs_f2 kQ67 = fg_load_cols<2, 3>(aKQ);  // (requested here: the registers of cL are free)
                        fg_load_slot<+1>(am1, u0, u1, u2);                                  // s6 (-1, +1)
                        FG_WAIT(3, v0, v1, v2);
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, fg_from_right(fg_from_right(scP1)));
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, fg_from_right(fg_from_right(scQ1)));
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<+1>(ap1, v0, v1, v2);                                  // s7 (+1, +1)
                        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(kQ67), "+v"(u0), "+v"(u1), "+v"(u2));
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, fg_from_left(scQ2));
                        {
                            const float sc = fg_scale(xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, sLQ[2], kQ67.x, l2a);
                            fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, sc);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // rest lengths and stiffness of the z-direction slots of rows P, Q from the row tables (stiffness 0 = row
                        // + dz outside the grid), requested only now, two slots at a time: the registers of the shear slots are
                        // free from here on
                        constexpr int KZ = FG_OFF_KZ - FG_OFF_ROWL;
                        fs_f2 zL[4], zK[4];
                        zL[0] = fg_load_rows<0>(aRow); zK[0] = fg_load_rows<KZ>(aRow);
                        zL[1] = fg_load_rows<256>(aRow); zK[1] = fg_load_rows<KZ + 256>(aRow);
                        fg_load_slot<-1>(a00, u0, u1, u2);                                  // s8 (0, -1)
                        asm volatile("s_waitcnt lgkmcnt(3)"
                                     : "+v"(zL[0]), "+v"(zK[0]), "+v"(zL[1]), "+v"(zK[1]), "+v"(v0), "+v"(v1), "+v"(v2));
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, fg_from_right(scQ3));
                        {
                            const float sc = fg_scale(xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, sLQ[3], kQ67.y, l2b);
                            fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, sc);
                        }
                        mQ = fminf(fminf(mQ, l2a), l2b);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<-2>(a00, v0, v1, v2);                                  // s9 (0, -2)
                        FG_WAIT(3, u0, u1, u2);
                        // Q's s8 (0, -1): the partner is P, in this thread's registers
                        const float scQ8 = fg_scale(xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, zL[0].y, zK[0].y, l2b);
                        {
                            const float sc = fg_scale(xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, zL[0].x, zK[0].x, l2a);
                            fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, sc);
                        }
                        fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, scQ8);
                        __builtin_amdgcn_sched_barrier(0);
                        zL[2] = fg_load_rows<512>(aRow); zK[2] = fg_load_rows<KZ + 512>(aRow);
                        zL[3] = fg_load_rows<768>(aRow); zK[3] = fg_load_rows<KZ + 768>(aRow);
                        fg_load_slot<+1>(a00, u0, u1, u2);                                  // s10 (0, +1)
                        asm volatile("s_waitcnt lgkmcnt(3)"
                                     : "+v"(zL[2]), "+v"(zK[2]), "+v"(zL[3]), "+v"(zK[3]), "+v"(v0), "+v"(v1), "+v"(v2));
                        {
                            const float sc = fg_scale(xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, zL[1].x, zK[1].x, l2c);
                            const float sd = fg_scale(xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, zL[1].y, zK[1].y, l2d);
                            fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, sc);
                            fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, sd);
                        }
                        mP = fminf(fminf(mP, l2a), l2c);
                        mQ = fminf(fminf(mQ, l2b), l2d);
                        __builtin_amdgcn_sched_barrier(0);
                        fg_load_slot<+2>(a00, v0, v1, v2);                                  // s11 (0, +2)
                        FG_WAIT(3, u0, u1, u2);
                        fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, u0.x, u1.x, u2.x, scQ8);
                        {
                            const float sd = fg_scale(xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, zL[2].y, zK[2].y, l2c);
                            fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, u0.y, u1.y, u2.y, sd);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        FG_WAIT(0, v0, v1, v2);
                        {
                            const float sc = fg_scale(xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, zL[3].x, zK[3].x, l2a);
                            const float sd = fg_scale(xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, zL[3].y, zK[3].y, l2b);
                            fg_accum(dP0, dP1, dP2, xi0.x, xi1.x, xi2.x, v0.x, v1.x, v2.x, sc);
                            fg_accum(dQ0, dQ1, dQ2, xi0.y, xi1.y, xi2.y, v0.y, v1.y, v2.y, sd);
                        }
                        mP = fminf(mP, l2a);
                        mQ = fminf(fminf(mQ, l2c), l2b);
                        __builtin_amdgcn_sched_barrier(0);
#undef FG_KX
                        // a coincident pair of particles (squared length 0, or below FG_MIN_L2: see fg_scale) takes the exact
                        // path instead.  The slots that took a shared scale add no squared length: the spring's evaluator --
                        // in the same wave and trip -- folded it, and a taken slot outside the grid adds the +0 of the DPP
                        // bound instead of k = 0.
                        exact = __builtin_amdgcn_ballot_w64(mP < FG_MIN_L2 || mQ < FG_MIN_L2) != 0ull;
                        aP = FsAcc{dP0, dP1, dP2, (int)((nvalid >> (16 * pr)) & 0xffu)};
                        aQ = FsAcc{dQ0, dQ1, dQ2, (int)((nvalid >> (16 * pr + 8)) & 0xffu)};
                    }
                    if (exact) {  // general form: the particle's ELL adjacency, fs_spring (any masses, zero lengths)
                        aP = FsAcc{0.0f, 0.0f, 0.0f, 0};
                        aQ = FsAcc{0.0f, 0.0f, 0.0f, 0};
                        if (haveP && wi.x > 0.0f)
                            for (int s = 0; s < max_deg; ++s) {
                                const int j = g_ell_j[(unsigned)s * un + (unsigned)iP];
                                if (j < 0) break;
                                fs_spring(aP, xi0.x, xi1.x, xi2.x, wi.x, FsVec4{Xx[j], Xy[j], Xz[j], Xw[j]},
                                          g_ell_len[(unsigned)s * un + (unsigned)iP], g_ell_k[(unsigned)s * un + (unsigned)iP]);
                            }
                        if (haveQ && wi.y > 0.0f)
                            for (int s = 0; s < max_deg; ++s) {
                                const int j = g_ell_j[(unsigned)s * un + (unsigned)iQ];
                                if (j < 0) break;
                                fs_spring(aQ, xi0.y, xi1.y, xi2.y, wi.y, FsVec4{Xx[j], Xy[j], Xz[j], Xw[j]},
                                          g_ell_len[(unsigned)s * un + (unsigned)iQ], g_ell_k[(unsigned)s * un + (unsigned)iQ]);
                            }
                    }
                    FS_TS(5)
                    // ---- park the sums of P, then Q: in the slot's accumulator for the contact phase, or in the trip's registers
                    const unsigned slw = pr == 0 ? slotw[0] : slotw[1];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int i = h == 0 ? iP : iQ;
                        FsAcc &a = h == 0 ? aP : aQ;
                        const unsigned myslot = h == 0 ? (slw & 0xffffu) : (slw >> 16);
                        if (myslot < FG_SLOT_INLINE) {
                            cacc[myslot] = FsVec4{a.d0, a.d1, a.d2, __int_as_float(a.cnt)};
                        } else if (myslot == FG_SLOT_INLINE) {  // candidates, but neither set nor queue had room (rare)
                            const float xi0s = h == 0 ? xi0.x : xi0.y, xi1s = h == 0 ? xi1.x : xi1.y, xi2s = h == 0 ? xi2.x : xi2.y;
                            const float wis = h == 0 ? wi.x : wi.y;
                            const float ri0 = xi0s - X0x[i], ri1 = xi1s - X0y[i], ri2 = xi2s - X0z[i];
                            const int cnt = g_ncount[i] & FS_NCOUNT_MASK;
#pragma unroll 1
                            for (int sq = 0; sq < cnt; ++sq) {
                                const int j = g_nlist[(unsigned)sq * un + (unsigned)i];
                                const FsVec4 xj = FsVec4{Xx[j], Xy[j], Xz[j], Xw[j]};
                                fs_particle_contact(a, xi0s, xi1s, xi2s, wis, ri0, ri1, ri2, xj, xj.x - X0x[j], xj.y - X0y[j],
                                                    xj.z - X0z[j], c.restd, c.restd2, c.mu_p);
                            }
                        }
                    }
                    // the only rotation: the trip before makes room (P and Q keep their names inside a trip)
#pragma unroll
                    for (int q = 0; q < 3; ++q) { rold[0][q] = rnew[0][q]; rold[1][q] = rnew[1][q]; }
                    rnew[0][0] = aP.d0; rnew[0][1] = aP.d1; rnew[0][2] = aP.d2;
                    rnew[1][0] = aQ.d0; rnew[1][1] = aQ.d1; rnew[1][2] = aQ.d2;
                    cpack = (cpack << 16) | ((unsigned)aP.cnt << 8) | (unsigned)aQ.cnt;
                    FS_TS(6)
                }
                __syncthreads();
                FS_TS(7)
                // ---- contact phase.  First the shape candidates of the thread's own particles for the finish phase: they
                // travel while the contacts are evaluated (iteration-invariant, but loaded here: four registers less across
                // the spring phase)
                unsigned smk[FS_FUSED_PPT];
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const int i = FG_ROW(w, k) * 64 + lane;
                    unsigned ic = i < n ? (unsigned)i : 0u;
                    asm volatile("" : "+v"(ic));  // keep the load inside the loop
                    smk[k] = (unsigned)g_ncount[ic] >> FS_SHAPE_MASK_SHIFT;
                }
                // the contact-set particle of this thread: its contacts in list order onto the parked sums
                if (i2 >= 0) {
                    const float xi0 = Xx[i2], xi1 = Xy[i2], xi2 = Xz[i2], wi = Xw[i2];
                    const FsVec4 pa = cacc[t];
                    FsAcc a = {pa.x, pa.y, pa.z, __float_as_int(pa.w)};
                    const float ri0 = xi0 - X0x[i2], ri1 = xi1 - X0y[i2], ri2 = xi2 - X0z[i2];
                    int cjt[FS_FUSED_PREFETCH_CAND];
#pragma unroll
                    for (int q = 0; q < FS_FUSED_PREFETCH_CAND; ++q) cjt[q] = cj2[q];
                    for (int s0 = 0; s0 < cnt2; s0 += FS_FUSED_PREFETCH_CAND) {
                        int cn[FS_FUSED_PREFETCH_CAND];
#pragma unroll
                        for (int q = 0; q < FS_FUSED_PREFETCH_CAND; ++q) {
                            const int sn = s0 + FS_FUSED_PREFETCH_CAND + q;
                            cn[q] = sn < cnt2 ? g_nlist[(unsigned)sn * un + (unsigned)i2] : 0;
                        }
#pragma unroll 1
                        for (int q = 0; q < FS_FUSED_PREFETCH_CAND && s0 + q < cnt2; ++q) {
                            const int j = cjt[0];
#pragma unroll
                            for (int r = 0; r + 1 < FS_FUSED_PREFETCH_CAND; ++r) cjt[r] = cjt[r + 1];
                            const FsVec4 xj = FsVec4{Xx[j], Xy[j], Xz[j], Xw[j]};
                            fs_particle_contact(a, xi0, xi1, xi2, wi, ri0, ri1, ri2, xj, xj.x - X0x[j], xj.y - X0y[j],
                                                xj.z - X0z[j], c.restd, c.restd2, c.mu_p);
                        }
#pragma unroll
                        for (int q = 0; q < FS_FUSED_PREFETCH_CAND; ++q) cjt[q] = cn[q];
                    }
                    cacc[t] = FsVec4{a.d0, a.d1, a.d2, __int_as_float(a.cnt)};
                }
#if FG_SINGLES
                // the overflow queue: entries q and q + 960 of waves 1..15
#pragma unroll 1
                for (int r = 0, q = t - 64; q >= 0 && q < n_singles; ++r, q += FG_SINGLES_LANES) {
                    const unsigned word = r == 0 ? qw0 : qw1;
                    const int i = (int)(word & 0xfffu), more = (int)(word >> 28);
                    int j = (int)((word >> 12) & 0xfffu);
                    int jn = more > 0 ? g_nlist[un + (unsigned)i] : 0;  // (the second candidate travels while the first is evaluated)
                    const FsVec4 pa = squeue[q];
                    FsAcc a = {pa.x, pa.y, pa.z, __float_as_int(pa.w)};
                    const float xi0 = Xx[i], xi1 = Xy[i], xi2 = Xz[i], wi = Xw[i];
                    const float ri0 = xi0 - X0x[i], ri1 = xi1 - X0y[i], ri2 = xi2 - X0z[i];
#pragma unroll 1
                    for (int sq = 0; sq <= more; ++sq) {
                        const FsVec4 xj = FsVec4{Xx[j], Xy[j], Xz[j], Xw[j]};
                        fs_particle_contact(a, xi0, xi1, xi2, wi, ri0, ri1, ri2, xj, xj.x - X0x[j], xj.y - X0y[j], xj.z - X0z[j], c.restd,
                                            c.restd2, c.mu_p);
                        j = jn;
                        if (sq + 2 <= more) jn = g_nlist[(unsigned)(sq + 2) * un + (unsigned)i];
                    }
                    squeue[q] = FsVec4{a.d0, a.d1, a.d2, __int_as_float(a.cnt)};
                }
#endif
                FS_TS(8)
                __syncthreads();  // every read of the old iterate is done, every accumulator complete
                FS_TS(9)
                // ---- finish phase: the thread's own four particles, a trip's P and Q in one body (h = 0: P, h = 1: Q; two
                // particles of the same thread, each reading and writing only its own state, so their instructions interleave
                // without changing a bit).  Per particle the order of fs_fused_shape_contacts: planes ascending, spheres
                // ascending, applyDeltas.
#pragma unroll 1
                for (int pr = 0; pr < 2; ++pr) {
                    const int iP = FG_ROW(w, 2 * pr) * 64 + lane;
                    const unsigned slw = pr == 0 ? slotw[0] : slotw[1];
                    FsAcc a[2];
                    unsigned sm[2];
                    bool act[2];
                    float x0[2], x1[2], x2[2], r0[2], r1[2], r2[2];
                    // the shape counts, routed through the trip as scalar registers so that they are tested here (s_cmp): as
                    // loop-invariant conditions they are hoisted out of every loop, kept as lane-mask pairs, and turned into a
                    // vector register and compared again at each use
                    int n_planes = c.n_planes, n_shapes = c.n_shapes;
                    asm volatile("" : "+s"(n_planes), "+s"(n_shapes));
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int i = iP + 64 * h;  // (below 4096 for every wave: rows past the cloth hold zeros)
                        const unsigned myslot = h == 0 ? (slw & 0xffffu) : (slw >> 16);
                        // a pinned particle (and a row past the cloth, whose inverse mass reads 0) stays where it is
                        act[h] = (i < n) & (Xw[i] > 0.0f);
                        // the sums: selected once, from the slot or from the registers of the older trip
                        a[h] = FsAcc{rold[h][0], rold[h][1], rold[h][2], (int)(h == 0 ? cpack >> 24 : (cpack >> 16) & 0xffu)};
                        if (act[h] && myslot < FG_SLOT_INLINE) {
                            const FsVec4 pa = cacc[myslot];
                            a[h] = FsAcc{pa.x, pa.y, pa.z, __float_as_int(pa.w)};
                        }
                        sm[h] = act[h] ? (pr == 0 ? smk[h] : smk[2 + h]) : 0u;
                        x0[h] = Xx[i]; x1[h] = Xy[i]; x2[h] = Xz[i];
                        r0[h] = x0[h] - X0x[i]; r1[h] = x1[h] - X0y[i]; r2[h] = x2[h] - X0z[i];
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q) { rold[0][q] = rnew[0][q]; rold[1][q] = rnew[1][q]; }
                    cpack <<= 16;
                    // planes
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        // (one after the other, not either / or: joined behind an else, the accumulator is copied into and
                        // out of the registers of the general loop on the single-plane path as well)
                        int q = 0;
                        if (n_planes == 1) {  // the ground alone: its coefficients are registers (c.pl* = planes[0])
                            if (sm[h] & 1u)
                                fs_plane_contact(a[h], x0[h], x1[h], x2[h], r0[h], r1[h], r2[h], c.pl0, c.pl1, c.pl2, c.pl3, c.cd, c.mu_s,
                                                 c.mu_k);
                            q = 1;
                        }
                        for (; q < n_planes; ++q)
                            if ((sm[h] >> q) & 1u)
                                fs_plane_contact(a[h], x0[h], x1[h], x2[h], r0[h], r1[h], r2[h], E.p.planes[q][0], E.p.planes[q][1],
                                                 E.p.planes[q][2], E.p.planes[q][3], c.cd, c.mu_s, c.mu_k);
                    }
                    // spheres: skipped by every wavefront none of whose lanes lists one for P or Q (all of them while the
                    // pickers are parked); a sphere's sweep and test run only where a lane lists it for that particle
                    if (n_shapes != 0 && __builtin_amdgcn_ballot_w64(((sm[0] | sm[1]) >> FS_SHAPE_SPHERE_BIT) != 0u) != 0ull) {
                        const float S = (float)c.substeps;
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            for (int q = 0; q < n_shapes; ++q)
                                if ((sm[h] >> (FS_SHAPE_SPHERE_BIT + q)) & 1u) {
                                    float c0, c1, c2, s0, s1, s2;
                                    fs_shape_sweep(sh, q, sub, S, c0, c1, c2, s0, s1, s2);
                                    fs_sphere_contact(a[h], x0[h], x1[h], x2[h], r0[h], r1[h], r2[h], c0, c1, c2, sh.pos[q].w, s0, s1, s2,
                                                      c.cd, c.mu_s, c.mu_k);
                                }
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (act[h]) {
                            const int i = iP + 64 * h;
                            fg_apply(a[h], c.relax, rcnt, x0[h], x1[h], x2[h]);
                            Xx[i] = x0[h]; Xy[i] = x1[h]; Xz[i] = x2[h];
                        }
                }
                __syncthreads();
                FS_TS(10)
            }
            // ---- finalize
            // The four velocities are one batch of loads with one wait; the results stay in registers as the next substep's
            // start (or the launch's result), and the velocity stores close the pass.  E.vel holds the new velocity when the
            // launch ends; inside the launch nobody reads it but this pass.
            {
                unsigned tl = (unsigned)t;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    sv[k] = fs_ld4o(E.vel, i < un ? i : 0u);
                }
                // the pass's constants, fetched together (they do not stay in registers across the iterations: taken one
                // by one where a particle uses them, each is a round trip of its own)
                FsFusedConsts cf = c;
                asm volatile("" : "+v"(cf.inv_h), "+v"(cf.maxdv2), "+v"(cf.maxdv), "+v"(cf.max_speed), "+v"(cf.thr2));
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    // (no test of i here: a slot past the cloth reads inverse mass 0 and takes the pinned exit, and nothing
                    // below uses what it leaves; assigned under a condition, sx would have to stay alive across the whole substep)
                    const FsVec4 xf = FsVec4{Xx[i], Xy[i], Xz[i], Xw[i]};
                    sx[k] = FsVec4{X0x[i], X0y[i], X0z[i], xf.w};
                    fs_fused_finalize(cf, sx[k], sv[k], xf);
                }
#pragma unroll
                for (int k = 0; k < FS_FUSED_PPT; ++k) {
                    const unsigned i = tl + (unsigned)(k * FS_FUSED_THREADS);
                    if (i < un) fs_st4o(E.vel, i, sv[k]);
                }
            }
        }
    }
    // the positions the last finalize left (for a launch of no substeps: the ones loaded)
#pragma unroll
    for (int k = 0; k < FS_FUSED_PPT; ++k) {
        const int i = t + k * FS_FUSED_THREADS;
        if (i < n) fs_st4o(g_pos, (unsigned)i, sx[k]);
    }
#ifdef FS_BLOCK_CLOCKS
    // Entry-to-exit shader clocks and the constant 100 MHz clock at entry / exit, left in row 95 of the episode's neighbour
    // table (no list of the bench reaches it; fs_get_last_neighbors of this build passes the row through).  Not printf:
    // workgroups that wait for the host to print slow down the ones still running by a factor of up to 7.
    if (t == 0) {
        const unsigned long long tc_total = __builtin_amdgcn_s_memtime() - tc_start, tr_end = __builtin_amdgcn_s_memrealtime();
        const fs_gi out = g_nlist + 95u * un;
        out[0] = (int)(unsigned)tc_total; out[1] = (int)(unsigned)(tc_total >> 32);
        out[2] = (int)(unsigned)tr_start; out[3] = (int)(unsigned)tr_end;
    }
#endif
#ifdef FS_TIMING
    FS_TS(11)
#ifdef FS_TIMING_COUNTS
    if (blockIdx.x == 0 && t == 0)
        printf("DBG runs(wave) %llu trips(wave) %llu candidates(lane) %llu survivors(lane) %llu accepted(lane) %llu phaseB trips(wave) %llu\n",
               fs_dbg_cnt[0], fs_dbg_cnt[1], fs_dbg_cnt[2], fs_dbg_cnt[3], fs_dbg_cnt[4], fs_dbg_cnt[5]);
#endif
    if (blockIdx.x == 0 && (t & 63) == 0)
        printf("TS wave %2d: init %llu predict %llu grid %llu find %llu findwait %llu sort %llu restore %llu alloc %llu cset %llu springs %llu park %llu bar1 %llu contact %llu bar2 %llu finish+bar3 %llu final %llu\n",
               t >> 6, ts_acc[0], ts_acc[12], ts_acc[1], ts_acc[2], ts_acc[3], ts_acc[15], ts_acc[13], ts_acc[14], ts_acc[4], ts_acc[5], ts_acc[6],
               ts_acc[7], ts_acc[8], ts_acc[9], ts_acc[10], ts_acc[11]);
#endif
}
