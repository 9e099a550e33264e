// What every grouped entry with a by-value link table decides on the host (dccn.h "the receive front end for several links",
// "classical receive"): the count, every link through its solo plan, the optional outputs (all links or none), and the one thing
// only a group can get wrong -- an output of one link meeting a range of another.  Host code only.
#pragma once
#include "common.h"

namespace dccn {

static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

// A link's byte ranges, outputs first: an output of one link must not meet ANY range of another (inputs may be shared).
struct LinkRanges {
    static constexpr int kMax = 16;
    const void* p[kMax];
    size_t n[kMax];
    int count = 0, outputs = 0;
    void out(const void* q, size_t bytes) { if (q) { p[count] = q; n[count++] = bytes; outputs = count; } }
    void in(const void* q, size_t bytes) { if (q) { p[count] = q; n[count++] = bytes; } }
};
static inline bool links_collide(const LinkRanges* r, int n_links) {
    for (int i = 0; i < n_links; ++i)
        for (int j = 0; j < n_links; ++j) {
            if (i == j) continue;
            for (int a = 0; a < r[i].outputs; ++a)
                for (int b = 0; b < r[j].count; ++b)
                    if (ranges_overlap(r[i].p[a], r[i].n[a], r[j].p[b], r[j].n[b])) return true;
        }
    return false;
}
// an optional output: given for every link or for none
template <class Link, class T>
static inline bool mixed_nullability(const Link* links, int n_links, T* Link::*field) {
    for (int i = 1; i < n_links; ++i)
        if ((links[i].*field == nullptr) != (links[0].*field == nullptr)) return true;
    return false;
}
// The plan of a group, stated once: the count, then per_link(i, link, ranges) for every link in order -- the link's solo plan, its
// entry of the launch's table, its byte ranges; the shape and the launch geometry are the call's, so every link's plan holds the
// same ones -- then the optional outputs (all links or none) and the collisions.
template <class Link, class PerLink, class... Optional>
static inline int group_plan(int n_links, const Link* links, PerLink per_link, Optional... optional) {
    if (n_links < 1 || n_links > kMaxChains || !links) return DCCN_ERR_INVALID_ARG;
    LinkRanges r[kMaxChains];
    for (int i = 0; i < n_links; ++i) DCCN_TRY(per_link(i, links[i], &r[i]));
    if ((mixed_nullability(links, n_links, optional) || ...)) return DCCN_ERR_INVALID_ARG;
    return links_collide(r, n_links) ? DCCN_ERR_INVALID_ARG : DCCN_OK;
}

}  // namespace dccn
