// Stand-alone host check of the sort pass's register network (csrc/fs_pair_search.h: fs_pair_sort16) and of the way the kernel
// uses it (fs_pair_sort_column in csrc/fs_fused_kernel.h): a column of `cnt` ids in any order, padded to 16 with FS_NB_EMPTY,
// comes out ascending with the pad behind it; longer columns take the in-place insertion sort restated here.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__host__= -D__device__= pair_sort_check.cpp
// Exit status 0 and "pair sort ok" when everything holds.  Runs on the CPU; nothing of it is loaded into python.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../flingbot_amd/csrc/fs_pair_search.h"

static const int EMPTY = 0x7fffffff;  // FS_NB_EMPTY

// a column of the neighbour table, n apart like the kernel's: sorted the way fs_pair_sort_column does it
static void sort_column(std::vector<int> &table, int n, int i, int cnt) {
    if (cnt < 1) return;
    int *col = table.data() + i;
    if (cnt <= FS_PAIR_SORT_BOUND) {
        int v[FS_PAIR_SORT_BOUND];
        const int last = cnt - 1;
        for (int a = 0; a < FS_PAIR_SORT_BOUND; ++a) v[a] = col[(size_t)std::min(a, last) * n];  // clamped, as the batch of loads
        for (int a = 1; a < FS_PAIR_SORT_BOUND; ++a)
            if (a >= cnt) v[a] = EMPTY;
        fs_pair_sort16(v);
        for (int a = 0; a < FS_PAIR_SORT_BOUND; ++a)
            if (a < cnt) col[(size_t)a * n] = v[a];
        return;
    }
    for (int a = 1; a < cnt; ++a) {
        const int v = col[(size_t)a * n];
        int b = a;
        while (b > 0) {
            const int p = col[(size_t)(b - 1) * n];
            if (p <= v) break;
            col[(size_t)b * n] = p;
            --b;
        }
        col[(size_t)b * n] = v;
    }
}

int main() {
    // the network itself, exhaustively: it sorts every 0/1 input, hence every input
    for (unsigned bits = 0; bits < (1u << FS_PAIR_SORT_BOUND); ++bits) {
        int v[FS_PAIR_SORT_BOUND];
        for (int a = 0; a < FS_PAIR_SORT_BOUND; ++a) v[a] = (bits >> a) & 1u;
        fs_pair_sort16(v);
        for (int a = 1; a < FS_PAIR_SORT_BOUND; ++a)
            if (v[a - 1] > v[a]) { std::printf("network fails on 0/1 input %#x\n", bits); return 1; }
    }
    // random columns of every length 0..96 among untouched neighbours
    std::mt19937 rng(12345);
    const int n = 7, cap = 96;
    for (int cnt = 0; cnt <= cap; ++cnt)
        for (int rep = 0; rep < 200; ++rep) {
            std::vector<int> table((size_t)cap * n, -7);
            const int i = (int)(rng() % n);
            std::vector<int> ids(4096);
            for (int q = 0; q < 4096; ++q) ids[q] = q;
            std::shuffle(ids.begin(), ids.end(), rng);
            std::vector<int> want(ids.begin(), ids.begin() + cnt);
            for (int a = 0; a < cnt; ++a) table[(size_t)a * n + i] = want[a];
            std::sort(want.begin(), want.end());
            sort_column(table, n, i, cnt);
            for (int a = 0; a < cap; ++a)
                for (int p = 0; p < n; ++p) {
                    const int expect = (p == i && a < cnt) ? want[a] : -7;
                    if (table[(size_t)a * n + p] != expect) {
                        std::printf("length %d: entry %d of column %d is %d, expected %d\n", cnt, a, p, table[(size_t)a * n + p], expect);
                        return 1;
                    }
                }
        }
    std::printf("pair sort ok\n");
    return 0;
}
