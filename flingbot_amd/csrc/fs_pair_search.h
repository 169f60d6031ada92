// fs_pair_search.h -- the enumeration rule of the half-stencil neighbour search (find mode 4 of fs_k_fused_grid64), shared
// by the kernel and by the host entry fs_host_pair_search, which runs the same rule on the CPU (tests/test_pair_search_cpu.py).
//
// Every unordered pair (i, j) with |x_i - x_j|^2 < radius^2 is found by exactly ONE of its endpoints, its owner, which appends
// it to both lists.  With cell(p) = floor(x * inv_rad) on the predicted positions, d = cell(j) - cell(i) and slot(p) = p's
// index in the bucket-ordered arrays, i owns (i, j) when
//     d is in {-1, 0, 1}^3 and (d.z, d.y, d.x) > (0, 0, 0) lexicographically  ("forward"),   or
//     d == 0 and slot(j) > slot(i).
// Exactly one endpoint owns every pair the full 27-cell search lists.  A hit whose true offset lies outside {-1, 0, 1}^3 (a
// hash alias in a rounding corner) is owned by nobody; the 27-cell search of true cells does not list it either.
//
// i therefore scans FIVE runs of the bucket-ordered arrays instead of nine:
//     run 0..2   rows (dy, dz) = (-1, +1), (0, +1), (+1, +1)     the full three-bucket run row(cy+dy, cz+dz) + cx-1 .. cx+1
//     run 3      row  (dy, dz) = (+1,  0)                        likewise
//     run 4      its own row, from slot(i) + 1 to the end of bucket row(cy, cz) + cx + 1
// and takes a hit only from the run whose (dy, dz) equals (d.y, d.z): two runs that overlap in bucket space through
// aliasing cannot produce a pair twice.
#pragma once

#define FS_PAIR_RUNS 5
#define FS_PAIR_OWN_RUN 4

// row hash of the LDS spatial hash: the cells (cx, cy, cz) of one row are the buckets (row + cx) mod 2^bits
__host__ __device__ inline int fs_pair_row(int cy, int cz, int bits) {
    const unsigned h = (unsigned)cy * 0x85EBCA77u + (unsigned)cz * 0xC2B2AE3Du;
    return (int)((h ^ (h >> 15)) * 0x2C1B3C6Du >> (32 - bits));
}

// (dy, dz) of run r
__host__ __device__ inline void fs_pair_run_row(int r, int &dy, int &dz) {
    dz = r < 3 ? 1 : 0;
    dy = r < 3 ? r - 1 : (r == 3 ? 1 : 0);
}

// Slot range [beg, end) of segment `seg` (0 or 1) of run r of the particle at slot `qs` in cell (cx, cy, cz); false when the
// run has no such segment.  cursor[b] = end of bucket b (its start is cursor[b - 1], 0 for b = 0).  A run whose buckets
// pass the end of the table continues at bucket 0: that is its second segment.
template <typename Cursor>
__host__ __device__ inline bool fs_pair_run_segment(const Cursor cursor, int bits, int r, int seg, int qs, int cx, int cy, int cz,
                                                    int &beg, int &end) {
    const int nb = 1 << bits;
    int dy, dz;
    fs_pair_run_row(r, dy, dz);
    const bool own = r == FS_PAIR_OWN_RUN;
    // first and last bucket of the run: cx - 1 .. cx + 1, the own row cx .. cx + 1
    const int b0 = (fs_pair_row(cy + dy, cz + dz, bits) + cx - (own ? 0 : 1)) & (nb - 1);
    const int wrap = b0 + (own ? 1 : 2) - (nb - 1);  // > 0: that many buckets continue at bucket 0
    if (seg == 0) {
        beg = own ? qs + 1 : (b0 == 0 ? 0 : (int)cursor[b0 - 1]);
        end = (int)cursor[wrap > 0 ? nb - 1 : b0 + (own ? 1 : 2)];
        return true;
    }
    if (wrap <= 0) return false;
    beg = 0;
    end = (int)cursor[wrap - 1];
    return true;
}

// Does the scan of run r take a hit whose true cell offset is (ddx, ddy, ddz) = cell(j) - cell(i)?  (In the own run every
// candidate of i's own cell already has slot(j) > slot(i): the run starts behind i.)
__host__ __device__ inline bool fs_pair_run_takes(int r, int ddx, int ddy, int ddz) {
    int dy, dz;
    fs_pair_run_row(r, dy, dz);
    if (ddy != dy || ddz != dz) return false;
    return r == FS_PAIR_OWN_RUN ? (unsigned)ddx <= 1u : (unsigned)(ddx + 1) <= 2u;
}

// the ownership rule itself, stated without runs (what the scan above implements)
__host__ __device__ inline bool fs_pair_owns(int ddx, int ddy, int ddz, int slot_i, int slot_j) {
    if ((unsigned)(ddx + 1) > 2u || (unsigned)(ddy + 1) > 2u || (unsigned)(ddz + 1) > 2u) return false;
    if (ddz != 0) return ddz > 0;
    if (ddy != 0) return ddy > 0;
    if (ddx != 0) return ddx > 0;
    return slot_j > slot_i;
}

// ---- the sort pass.  The owner appends a pair unsorted to both lists; afterwards every list is sorted ascending.
// FS_PAIR_HEADS: the first entries of a list (appends k < FS_PAIR_HEADS) are kept in LDS until the sort pass.
// FS_PAIR_SORT_BOUND: a list of up to this many entries is sorted in registers, by fs_pair_sort16; longer ones in place.
#define FS_PAIR_HEADS 4
#define FS_PAIR_SORT_BOUND 16
#define FS_PAIR_SORT16_STEPS 63

// Sorts v[0..15] ascending: Batcher's odd-even merge sort as a fixed network of 63 compare-exchanges (ten layers), every
// index a constant once the loop is unrolled, so v stays in registers.  A shorter list is padded with a value above every id.
__host__ __device__ inline void fs_pair_sort16(int (&v)[FS_PAIR_SORT_BOUND]) {
    constexpr unsigned char A[FS_PAIR_SORT16_STEPS] = {0, 2, 4, 6, 8, 10, 12, 14, 0, 1, 4, 5, 8, 9, 12, 13, 1, 5, 9, 13, 0,
                                                       1, 2, 3, 8, 9, 10, 11, 2, 3, 10, 11, 1, 3, 5, 9, 11, 13, 0, 1, 2, 3,
                                                       4, 5, 6, 7, 4, 5, 6, 7, 2, 3, 6, 7, 10, 11, 1, 3, 5, 7, 9, 11, 13};
    constexpr unsigned char B[FS_PAIR_SORT16_STEPS] = {1, 3, 5, 7, 9, 11, 13, 15, 2, 3, 6, 7, 10, 11, 14, 15, 2, 6, 10, 14, 4,
                                                       5, 6, 7, 12, 13, 14, 15, 4, 5, 12, 13, 2, 4, 6, 10, 12, 14, 8, 9, 10, 11,
                                                       12, 13, 14, 15, 8, 9, 10, 11, 4, 5, 8, 9, 12, 13, 2, 4, 6, 8, 10, 12, 14};
#pragma unroll
    for (int q = 0; q < FS_PAIR_SORT16_STEPS; ++q) {
        const int lo = v[A[q]] < v[B[q]] ? v[A[q]] : v[B[q]], hi = v[A[q]] < v[B[q]] ? v[B[q]] : v[A[q]];
        v[A[q]] = lo;
        v[B[q]] = hi;
    }
}
