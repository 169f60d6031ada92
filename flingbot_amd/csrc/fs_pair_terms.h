// fs_pair_terms.h -- the arithmetic of ONE pair of the pairwise ranking term, shared by fs_k_group_loss (fs_grouploss.hip) and
// fs_k_map_loss_pairs (fs_maploss.hip); include/flingsim.h has the rule.
//
// The pair's argument x = -margin / tau, margin = p_winner - p_loser, is formed in double ((double)p_i - (double)p_j is exact)
// and split into a float head and a float tail: exp(-|x|) = expf(-head) * (1 - tail).  In plain fp32 the rounding of x alone
// would put |x| ulp on exp(-|x|); with the tail every addend is good to a few ulp whatever |x| is.
// softplus(x) = max(x, 0) + log1p(e); sigma(x) = 1 / (1 + e) for x >= 0 and e / (1 + e) below, e = exp(-|x|): nothing overflows,
// |x| = 1e4 gives e = 0.
#pragma once
#include <hip/hip_runtime.h>

struct fs_pair_terms {
    double x;   // -margin / tau
    float e;    // exp(-|x|)
    float sig;  // sigma(x)
};

__device__ __forceinline__ fs_pair_terms fs_pair_eval(double margin, double inv_tau) {
    fs_pair_terms t;
    t.x = -(margin * inv_tau);
    const double ax = fabs(t.x);
    const float head = (float)ax;
    const float tail = head < 3.0e38f ? (float)(ax - (double)head) : 0.0f;  // (|x| past the floats: e = 0 all the same)
    t.e = expf(-head) * (1.0f - tail);
    const float inv = 1.0f / (1.0f + t.e);
    t.sig = t.x >= 0.0 ? inv : t.e * inv;
    return t;
}

__device__ __forceinline__ float fs_pair_softplus(const fs_pair_terms &t) { return fmaxf((float)t.x, 0.0f) + log1pf(t.e); }
