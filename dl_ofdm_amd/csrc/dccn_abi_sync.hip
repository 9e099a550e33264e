// libdccn.so -- per-frame timing alignment from the cyclic prefix (see abi_impl.h for how the library is cut into units)
#include <math.h>

#include "capture_acquire.h"
#include "common.h"
#include "frame_sync.h"

using namespace dccn;

namespace {
// Everything a call decides, before its one launch: a refused call launches nothing.
struct FrameSyncPlan {
    FrameSyncArgs args;
    unsigned blocks;
    size_t lds;
};

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

int frame_sync_plan(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                    float* metric, FrameSyncPlan* plan) {
    if (!frame_sync_shape_ok(S, K, CP, W) || frames <= 0 || !x || !offset) return DCCN_ERR_INVALID_ARG;
    if (out_kin != K + CP && out_kin != K) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(x) || !aligned16(x_out) || !aligned16(metric)) return DCCN_ERR_INVALID_ARG;
    const int T = S * (K + CP);
    // the cropped rows leave as 16-byte stores too: S * K complex samples per frame, an even count
    if (x_out && out_kin == K && (S * K) % 2 != 0) return DCCN_ERR_INVALID_ARG;
    if (x_out && ranges_overlap(x, (size_t)frames * T * 8, x_out, (size_t)frames * S * out_kin * 8)) return DCCN_ERR_INVALID_ARG;
    plan->args = FrameSyncArgs{x, x_out, offset, metric, frames, S, K, CP, W, out_kin == K ? 1 : 0};
    plan->blocks = (unsigned)ceil_div(frames, kSyncWaves);
    plan->lds = kSyncWaves * frame_sync_lds_per_frame(T);
    return DCCN_OK;
}

struct CaptureSyncPlan {
    CaptureSyncArgs args;
    unsigned blocks;
    size_t lds;
};

// sample_bytes: 8 for a float32 capture; 4 for an sc16 one, whose entries pass the capture's address as `cap` for the checks (the
// capture's extent is n_samples * sample_bytes) and launch kernels that do not read args.cap
int capture_sync_plan(const float* cap, long long n_samples, long long first, long long stride, int frames, int S, int K, int CP,
                      int W, int out_kin, float* x_out, int32_t* offset, float* cfo, float* metric, CaptureSyncPlan* plan,
                      size_t sample_bytes = 8) {
    if (!capture_sync_shape_ok(S, K, CP, W) || frames <= 0 || !cap || !offset) return DCCN_ERR_INVALID_ARG;
    if (out_kin != K + CP && out_kin != K) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(cap) || !aligned16(x_out) || !aligned16(metric)) return DCCN_ERR_INVALID_ARG;
    const long long T = (long long)S * (K + CP);
    if (x_out && out_kin == K && (S * K) % 2 != 0) return DCCN_ERR_INVALID_ARG;
    // every window [b_f - W, b_f + T + W) inside the capture, frames not overlapping: first - W >= 0 and
    // first + (frames - 1) stride + T + W <= n_samples, the product taken as a quotient so nothing overflows
    if (n_samples <= 0 || n_samples > (1LL << 58) || stride < T || first < W || first > n_samples) return DCCN_ERR_INVALID_ARG;
    const long long room = n_samples - first - T - W;
    if (room < 0 || (frames > 1 && stride > room / (frames - 1))) return DCCN_ERR_INVALID_ARG;
    if (x_out && ranges_overlap(cap, (size_t)n_samples * sample_bytes, x_out, (size_t)frames * S * out_kin * 8))
        return DCCN_ERR_INVALID_ARG;
    plan->args = CaptureSyncArgs{cap, first, stride, x_out, offset, metric, cfo, frames, S, K, CP, W, out_kin == K ? 1 : 0};
    plan->blocks = (unsigned)ceil_div(frames, kSyncWaves);
    plan->lds = kSyncWaves * capture_sync_lds_per_frame((int)T, W);
    return DCCN_OK;
}

template <bool CFO>
int capture_sync_launch(const CaptureSyncPlan& plan, dccn_stream_t stream) {
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_kernel<CFO>, plan.lds));
    hipLaunchKernelGGL(capture_sync_kernel<CFO>, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream,
                       plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
// dccn_capture_sync_at: the plan of dccn_capture_sync for the LAST start the kernel can clamp to (lo + T - 1: every earlier one
// has its windows inside the capture too, down to lo, whose first window starts at lo - W >= 0)
int capture_sync_at_plan(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                         int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                         float* metric, CaptureSyncPlan* plan, size_t sample_bytes = 8) {
    if (!capture_sync_shape_ok(S, K, CP, W) || !first_dev || (reinterpret_cast<uintptr_t>(first_dev) & 7u) != 0) return DCCN_ERR_INVALID_ARG;
    if (lo < W || n_samples <= 0 || lo > n_samples) return DCCN_ERR_INVALID_ARG;
    const long long T = (long long)S * (K + CP);
    return capture_sync_plan(cap, n_samples, lo + T - 1, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo, metric, plan,
                             sample_bytes);
}

template <bool CFO>
int capture_sync_at_launch(const CaptureSyncPlan& plan, const long long* first_dev, long long lo, dccn_stream_t stream) {
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_at_kernel<CFO>, plan.lds));
    hipLaunchKernelGGL(capture_sync_at_kernel<CFO>, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream,
                       CaptureSyncAtArgs{plan.args, first_dev, lo});
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// the wide cuts' two device inputs (acquisition's m^ and eps^): given, on 4-byte boundaries
bool wide_inputs_ok(const int32_t* cfo_int_dev, const float* cfo_frac_dev) {
    return cfo_int_dev && cfo_frac_dev && (reinterpret_cast<uintptr_t>(cfo_int_dev) & 3u) == 0 &&
           (reinterpret_cast<uintptr_t>(cfo_frac_dev) & 3u) == 0;
}

// Everything dccn_capture_acquire decides, before its first launch.
struct CaptureAcquirePlan {
    AcqArgs args;
    unsigned sum_blocks;
    size_t lds;
};

int capture_acquire_plan(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                         int n_pilot, long long* first_out, float* cfo_out, float* sym_metric, float* phase_metric,
                         void* workspace, size_t workspace_bytes, CaptureAcquirePlan* plan) {
    if (!capture_acquire_shape_ok(S, K, CP, n_pilot, J)) return DCCN_ERR_INVALID_ARG;
    if (!cap || !pilot_sc || !first_out || !cfo_out || !workspace) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(cap) || !aligned16(workspace) || (reinterpret_cast<uintptr_t>(first_out) & 7u) != 0) return DCCN_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(pilot_sc) & 3u) != 0 || (reinterpret_cast<uintptr_t>(cfo_out) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(sym_metric) & 3u) != 0 || (reinterpret_cast<uintptr_t>(phase_metric) & 3u) != 0)
        return DCCN_ERR_INVALID_ARG;
    // every read of both stages lies in [lo, lo + (J + 1) T); the documented bound leaves a frame to spare
    const long long T = (long long)S * (K + CP);
    if (lo < 0 || n_samples <= 0 || n_samples > (1LL << 58) || lo > n_samples || (J + 2) * T > n_samples - lo) return DCCN_ERR_INVALID_ARG;
    const AcqWorkspace w = capture_acquire_layout(S, K, CP, J);
    if (workspace_bytes < w.total) return DCCN_ERR_WORKSPACE;
    char* const base = static_cast<char*>(workspace);
    plan->args = AcqArgs{cap, lo, pilot_sc, reinterpret_cast<float4*>(base + w.pe), reinterpret_cast<float*>(base + w.partial),
                         reinterpret_cast<int*>(base + w.rhat), first_out, cfo_out, sym_metric, phase_metric, S, K, CP, J, n_pilot};
    plan->sum_blocks = (unsigned)ceil_div(K + 2 * CP - 1, kAcqSumThreads);
    plan->lds = capture_acquire_lds(S, K, CP, n_pilot);
    return DCCN_OK;
}

// ---- the grouped entries: every link through the solo plan above, then what only a group can get wrong --------------------------
// A link's byte ranges, outputs first: an output of one link must not meet ANY range of another (inputs may be shared).
struct LinkRanges {
    static constexpr int kMax = 8;
    const void* p[kMax];
    size_t n[kMax];
    int count = 0, outputs = 0;
    void out(const void* q, size_t bytes) { if (q) { p[count] = q; n[count++] = bytes; outputs = count; } }
    void in(const void* q, size_t bytes) { if (q) { p[count] = q; n[count++] = bytes; } }
};
bool links_collide(const LinkRanges* r, int n_links) {
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
bool mixed_nullability(const Link* links, int n_links, T* Link::*field) {
    for (int i = 1; i < n_links; ++i)
        if ((links[i].*field == nullptr) != (links[0].*field == nullptr)) return true;
    return false;
}
bool group_count_ok(int n_links, const void* links) { return n_links >= 1 && n_links <= kMaxChains && links != nullptr; }

struct FrameSyncGroupPlan {
    FrameSyncGroupArgs args;
    unsigned blocks;
    size_t lds;
    bool cfo;
};
int frame_sync_group_plan(int n_links, const dccn_frame_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                          FrameSyncGroupPlan* plan) {
    if (!group_count_ok(n_links, links)) return DCCN_ERR_INVALID_ARG;
    LinkRanges r[kMaxChains];
    plan->args = FrameSyncGroupArgs{};
    for (int i = 0; i < n_links; ++i) {
        const dccn_frame_link& l = links[i];
        FrameSyncPlan one;
        DCCN_TRY(frame_sync_plan(l.x, frames, S, K, CP, W, out_kin, l.x_out, l.offset, l.metric, &one));
        if ((reinterpret_cast<uintptr_t>(l.cfo) & 3u) != 0) return DCCN_ERR_INVALID_ARG;
        plan->args.link[i] = FrameSyncLink{one.args.x, one.args.x_out, one.args.offset, one.args.metric, l.cfo};
        if (i == 0) {
            plan->args.frames = frames; plan->args.S = S; plan->args.K = K; plan->args.CP = CP; plan->args.W = W;
            plan->args.crop = one.args.crop;
            plan->blocks = one.blocks;
            plan->lds = one.lds;
        }
        r[i].out(l.x_out, (size_t)frames * S * out_kin * 8);
        r[i].out(l.offset, (size_t)frames * 4);
        r[i].out(l.cfo, (size_t)frames * 4);
        r[i].out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r[i].in(l.x, (size_t)frames * S * (K + CP) * 8);
    }
    if (mixed_nullability(links, n_links, &dccn_frame_link::x_out) || mixed_nullability(links, n_links, &dccn_frame_link::cfo) ||
        mixed_nullability(links, n_links, &dccn_frame_link::metric))
        return DCCN_ERR_INVALID_ARG;
    if (links_collide(r, n_links)) return DCCN_ERR_INVALID_ARG;
    plan->cfo = links[0].cfo != nullptr;
    return DCCN_OK;
}

struct CaptureSyncGroupPlan {
    CaptureSyncGroupArgs args;
    unsigned blocks;
    size_t lds;
    bool cfo;
};
int capture_sync_group_plan(int n_links, const dccn_capture_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                            CaptureSyncGroupPlan* plan) {
    if (!group_count_ok(n_links, links)) return DCCN_ERR_INVALID_ARG;
    LinkRanges r[kMaxChains];
    plan->args = CaptureSyncGroupArgs{};
    for (int i = 0; i < n_links; ++i) {
        const dccn_capture_link& l = links[i];
        CaptureSyncPlan one;
        if (l.first_dev)
            DCCN_TRY(capture_sync_at_plan(l.cap, l.n_samples, l.first_dev, l.lo, l.stride, frames, S, K, CP, W, out_kin, l.x_out,
                                          l.offset, l.cfo, l.metric, &one));
        else
            DCCN_TRY(capture_sync_plan(l.cap, l.n_samples, l.first, l.stride, frames, S, K, CP, W, out_kin, l.x_out, l.offset, l.cfo,
                                       l.metric, &one));
        if ((reinterpret_cast<uintptr_t>(l.cfo) & 3u) != 0) return DCCN_ERR_INVALID_ARG;
        plan->args.link[i] = CaptureSyncLink{one.args.cap, l.first_dev ? 0 : l.first, one.args.stride, l.first_dev,
                                             l.first_dev ? l.lo : 0, one.args.x_out, one.args.offset, one.args.metric, one.args.cfo};
        if (i == 0) {
            plan->args.frames = frames; plan->args.S = S; plan->args.K = K; plan->args.CP = CP; plan->args.W = W;
            plan->args.crop = one.args.crop;
            plan->blocks = one.blocks;
            plan->lds = one.lds;
        }
        r[i].out(l.x_out, (size_t)frames * S * out_kin * 8);
        r[i].out(l.offset, (size_t)frames * 4);
        r[i].out(l.cfo, (size_t)frames * 4);
        r[i].out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r[i].in(l.cap, (size_t)l.n_samples * 8);
        r[i].in(l.first_dev, 8);
    }
    if (mixed_nullability(links, n_links, &dccn_capture_link::x_out) || mixed_nullability(links, n_links, &dccn_capture_link::cfo) ||
        mixed_nullability(links, n_links, &dccn_capture_link::metric))
        return DCCN_ERR_INVALID_ARG;
    if (links_collide(r, n_links)) return DCCN_ERR_INVALID_ARG;
    plan->cfo = links[0].cfo != nullptr;
    return DCCN_OK;
}

// dccn_capture_sync_pooled(_grouped): every link through the per-frame entry's own plan (so the windows, the alignment and the
// cap / x_out overlap are judged by the same code), then what the pooled call adds.
size_t pooled_workspace_bytes(int frames) { return frames > 0 ? ((size_t)frames * sizeof(float2) + 15) & ~(size_t)15 : 0; }

struct PooledGroupPlan {
    PooledGroupArgs args;
    unsigned blocks;
    size_t lds_estimate, lds_cut;
};
int pooled_group_plan(int n_links, const dccn_pooled_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                      PooledGroupPlan* plan, size_t sample_bytes = 8) {
    if (!group_count_ok(n_links, links)) return DCCN_ERR_INVALID_ARG;
    LinkRanges r[kMaxChains];
    plan->args = PooledGroupArgs{};
    for (int i = 0; i < n_links; ++i) {
        const dccn_pooled_link& l = links[i];
        CaptureSyncPlan one;
        if (l.first_dev)
            DCCN_TRY(capture_sync_at_plan(l.cap, l.n_samples, l.first_dev, l.lo, l.stride, frames, S, K, CP, W, out_kin, l.x_out,
                                          l.offset, l.cfo, l.metric, &one, sample_bytes));
        else
            DCCN_TRY(capture_sync_plan(l.cap, l.n_samples, l.first, l.stride, frames, S, K, CP, W, out_kin, l.x_out, l.offset, l.cfo,
                                       l.metric, &one, sample_bytes));
        if (!l.x_out || !l.cfo || (reinterpret_cast<uintptr_t>(l.cfo) & 3u) != 0) return DCCN_ERR_INVALID_ARG;
        if (!l.workspace || !aligned16(l.workspace)) return DCCN_ERR_INVALID_ARG;
        plan->args.link[i] = PooledLink{CaptureSyncLink{one.args.cap, l.first_dev ? 0 : l.first, one.args.stride, l.first_dev,
                                                        l.first_dev ? l.lo : 0, one.args.x_out, one.args.offset, one.args.metric,
                                                        one.args.cfo},
                                        static_cast<float2*>(l.workspace)};
        if (i == 0) {
            plan->args.frames = frames; plan->args.S = S; plan->args.K = K; plan->args.CP = CP; plan->args.W = W;
            plan->args.crop = one.args.crop;
            plan->blocks = one.blocks;
            plan->lds_estimate = one.lds;
            plan->lds_cut = kSyncWaves * capture_cut_lds_per_frame(S * (K + CP));
        }
        r[i].out(l.x_out, (size_t)frames * S * out_kin * 8);
        r[i].out(l.offset, (size_t)frames * 4);
        r[i].out(l.cfo, 4);
        r[i].out(l.metric, (size_t)frames * (2 * W + 1) * 4);
        r[i].out(l.workspace, pooled_workspace_bytes(frames));
        r[i].in(l.cap, (size_t)l.n_samples * sample_bytes);
        r[i].in(l.first_dev, 8);
    }
    if (mixed_nullability(links, n_links, &dccn_pooled_link::metric)) return DCCN_ERR_INVALID_ARG;
    if (links_collide(r, n_links)) return DCCN_ERR_INVALID_ARG;
    for (int i = 0; i < n_links; ++i)
        if (links[i].workspace_bytes < pooled_workspace_bytes(frames)) return DCCN_ERR_WORKSPACE;
    return DCCN_OK;
}
int pooled_group_launch(const PooledGroupPlan& plan, int n_links, dccn_stream_t stream) {
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_estimate_kernel, plan.lds_estimate));
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_cut_kernel<PooledGroupArgs>, plan.lds_cut));
    const dim3 grid(plan.blocks, (unsigned)n_links), block(kSyncWaves * kSyncLanes);
    hipLaunchKernelGGL(capture_pool_estimate_kernel, grid, block, plan.lds_estimate, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_reduce_kernel, dim3((unsigned)n_links), dim3(kSyncLanes), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_cut_kernel<PooledGroupArgs>, grid, block, plan.lds_cut, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

struct CaptureAcquireGroupPlan {
    AcqGroupArgs args;
    unsigned sum_blocks;
    size_t lds;
};
int capture_acquire_group_plan(int n_links, const dccn_acquire_link* links, int J, int S, int K, int CP, int n_pilot,
                               CaptureAcquireGroupPlan* plan) {
    if (!group_count_ok(n_links, links)) return DCCN_ERR_INVALID_ARG;
    LinkRanges r[kMaxChains];
    plan->args = AcqGroupArgs{};
    for (int i = 0; i < n_links; ++i) {
        const dccn_acquire_link& l = links[i];
        CaptureAcquirePlan one;
        DCCN_TRY(capture_acquire_plan(l.cap, l.n_samples, l.lo, J, S, K, CP, l.pilot_sc, n_pilot, l.first_out, l.cfo_out, l.sym_metric,
                                      l.phase_metric, l.workspace, l.workspace_bytes, &one));
        const AcqArgs& a = one.args;
        plan->args.link[i] = AcqLink{a.cap, a.lo, a.pilot_sc, a.pe, a.partial, a.rhat, a.first_out, a.cfo_out, a.sym_metric,
                                     a.phase_metric};
        if (i == 0) {
            plan->args.S = S; plan->args.K = K; plan->args.CP = CP; plan->args.J = J; plan->args.n_pilot = n_pilot;
            plan->sum_blocks = one.sum_blocks;
            plan->lds = one.lds;
        }
        r[i].out(l.first_out, 8);
        r[i].out(l.cfo_out, 4);
        r[i].out(l.sym_metric, (size_t)(K + CP) * 4);
        r[i].out(l.phase_metric, (size_t)S * 4);
        r[i].out(l.workspace, capture_acquire_layout(S, K, CP, J).total);
        r[i].in(l.cap, (size_t)l.n_samples * 8);
        r[i].in(l.pilot_sc, (size_t)n_pilot * 4);
    }
    if (mixed_nullability(links, n_links, &dccn_acquire_link::sym_metric) ||
        mixed_nullability(links, n_links, &dccn_acquire_link::phase_metric))
        return DCCN_ERR_INVALID_ARG;
    if (links_collide(r, n_links)) return DCCN_ERR_INVALID_ARG;
    return DCCN_OK;
}

template <bool CFO>
int frame_sync_group_launch(const FrameSyncGroupPlan& plan, int n_links, dccn_stream_t stream) {
    DCCN_TRY(set_max_dynamic_smem((const void*)frame_sync_grouped_kernel<CFO>, plan.lds));
    hipLaunchKernelGGL(frame_sync_grouped_kernel<CFO>, dim3(plan.blocks, (unsigned)n_links), dim3(kSyncWaves * kSyncLanes), plan.lds,
                       (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
template <bool CFO>
int capture_sync_group_launch(const CaptureSyncGroupPlan& plan, int n_links, dccn_stream_t stream) {
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_grouped_kernel<CFO>, plan.lds));
    hipLaunchKernelGGL(capture_sync_grouped_kernel<CFO>, dim3(plan.blocks, (unsigned)n_links), dim3(kSyncWaves * kSyncLanes),
                       plan.lds, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- 16-bit integer I/Q captures: the float32 plans with the capture's extent taken as 4 bytes per sample -----------------------
bool sc16_scale_ok(float scale) { return isfinite(scale) && scale > 0.f; }
const float* sc16_as_checked(const int16_t* cap) { return reinterpret_cast<const float*>(cap); }    // (an address to check, never read)
}  // namespace

extern "C" {

int dccn_frame_sync_supported(int S, int K, int CP, int W) { return frame_sync_shape_ok(S, K, CP, W) ? 1 : 0; }

int dccn_frame_sync(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                    float* metric, dccn_stream_t stream) {
    FrameSyncPlan plan;
    DCCN_TRY(frame_sync_plan(x, frames, S, K, CP, W, out_kin, x_out, offset, metric, &plan));
    DCCN_TRY(set_max_dynamic_smem((const void*)frame_sync_kernel, plan.lds));
    hipLaunchKernelGGL(frame_sync_kernel, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream,
                       plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_frame_sync_cfo(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                        float* cfo, float* metric, dccn_stream_t stream) {
    FrameSyncPlan plan;
    DCCN_TRY(frame_sync_plan(x, frames, S, K, CP, W, out_kin, x_out, offset, metric, &plan));
    if (!cfo) return DCCN_ERR_INVALID_ARG;
    DCCN_NO_CHAINS();                         // (the launch carries no chain table: inside a group it would serve chain 0 only)
    DCCN_TRY(set_max_dynamic_smem((const void*)frame_sync_cfo_kernel, plan.lds));
    hipLaunchKernelGGL(frame_sync_cfo_kernel, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream,
                       FrameSyncCfoArgs{plan.args, cfo});
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_capture_sync_supported(int S, int K, int CP, int W) { return capture_sync_shape_ok(S, K, CP, W) ? 1 : 0; }

int dccn_capture_sync(const float* cap, long long n_samples, long long first, long long stride, int frames, int S, int K, int CP,
                      int W, int out_kin, float* x_out, int32_t* offset, float* cfo, float* metric, dccn_stream_t stream) {
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_plan(cap, n_samples, first, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo, metric, &plan));
    DCCN_NO_CHAINS();
    return cfo ? capture_sync_launch<true>(plan, stream) : capture_sync_launch<false>(plan, stream);
}

int dccn_capture_sync_at(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                         int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                         float* metric, dccn_stream_t stream) {
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_at_plan(cap, n_samples, first_dev, lo, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo, metric,
                                  &plan));
    DCCN_NO_CHAINS();
    return cfo ? capture_sync_at_launch<true>(plan, first_dev, lo, stream) : capture_sync_at_launch<false>(plan, first_dev, lo, stream);
}

int dccn_capture_acquire_supported(int S, int K, int CP, int n_pilot, int J) {
    return capture_acquire_shape_ok(S, K, CP, n_pilot, J) ? 1 : 0;
}

size_t dccn_capture_acquire_workspace_size(int S, int K, int CP, int n_pilot, int J) {
    return capture_acquire_shape_ok(S, K, CP, n_pilot, J) ? capture_acquire_layout(S, K, CP, J).total : 0;
}

int dccn_capture_acquire(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                         int n_pilot, long long* first_out, float* cfo_out, float* sym_metric, float* phase_metric,
                         void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    CaptureAcquirePlan plan;
    DCCN_TRY(capture_acquire_plan(cap, n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric, phase_metric,
                                  workspace, workspace_bytes, &plan));
    DCCN_NO_CHAINS();
    hipLaunchKernelGGL(acq_symbol_sums_kernel, dim3(plan.sum_blocks), dim3(kAcqSumThreads), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_phase_kernel, dim3((unsigned)S, (unsigned)J), dim3(kAcqThreads), plan.lds, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_decide_kernel, dim3(1), dim3(kAcqMaxS), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- several links per launch: the link table is the call's own, so inside a ChainScope these refuse like the solo entries ----
int dccn_frame_sync_grouped(int n_links, const dccn_frame_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                            dccn_stream_t stream) {
    FrameSyncGroupPlan plan;
    DCCN_TRY(frame_sync_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    return plan.cfo ? frame_sync_group_launch<true>(plan, n_links, stream) : frame_sync_group_launch<false>(plan, n_links, stream);
}

int dccn_capture_sync_grouped(int n_links, const dccn_capture_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                              dccn_stream_t stream) {
    CaptureSyncGroupPlan plan;
    DCCN_TRY(capture_sync_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    return plan.cfo ? capture_sync_group_launch<true>(plan, n_links, stream) : capture_sync_group_launch<false>(plan, n_links, stream);
}

int dccn_capture_acquire_grouped(int n_links, const dccn_acquire_link* links, int J, int S, int K, int CP, int n_pilot,
                                 dccn_stream_t stream) {
    CaptureAcquireGroupPlan plan;
    DCCN_TRY(capture_acquire_group_plan(n_links, links, J, S, K, CP, n_pilot, &plan));
    DCCN_NO_CHAINS();
    const unsigned G = (unsigned)n_links;
    hipLaunchKernelGGL(acq_symbol_sums_grouped_kernel, dim3(plan.sum_blocks, G), dim3(kAcqSumThreads), 0, (hipStream_t)stream,
                       plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_phase_grouped_kernel, dim3((unsigned)S, (unsigned)J, G), dim3(kAcqThreads), plan.lds, (hipStream_t)stream,
                       plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_decide_grouped_kernel, dim3(G), dim3(kAcqMaxS), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- one carrier offset per capture: the solo entry is the grouped one with one link -----------------------------------------
size_t dccn_capture_sync_pooled_workspace_size(int frames) { return pooled_workspace_bytes(frames); }

int dccn_capture_sync_pooled_grouped(int n_links, const dccn_pooled_link* links, int frames, int S, int K, int CP, int W,
                                     int out_kin, dccn_stream_t stream) {
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(n_links, links, frames, S, K, CP, W, out_kin, &plan));
    DCCN_NO_CHAINS();
    return pooled_group_launch(plan, n_links, stream);
}

int dccn_capture_sync_pooled(const float* cap, long long n_samples, long long first, const long long* first_dev, long long lo,
                             long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                             float* cfo_out, float* metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    const dccn_pooled_link link{cap, n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace, workspace_bytes};
    return dccn_capture_sync_pooled_grouped(1, &link, frames, S, K, CP, W, out_kin, stream);
}

// ---- 16-bit integer I/Q captures, converted inside the launches ----------------------------------------------------------------
int dccn_capture_sync_sc16(const int16_t* cap, long long n_samples, float scale, long long first, const long long* first_dev,
                           long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                           int32_t* offset, float* cfo, float* metric, dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    CaptureSyncPlan plan;
    if (first_dev)
        DCCN_TRY(capture_sync_at_plan(sc16_as_checked(cap), n_samples, first_dev, lo, stride, frames, S, K, CP, W, out_kin, x_out,
                                      offset, cfo, metric, &plan, 4));
    else
        DCCN_TRY(capture_sync_plan(sc16_as_checked(cap), n_samples, first, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo,
                                   metric, &plan, 4));
    DCCN_NO_CHAINS();
    plan.args.cap = nullptr;
    plan.args.first = first_dev ? 0 : first;
    const CaptureSyncSc16Args args{plan.args, CapSc16{cap, scale}, first_dev, first_dev ? lo : 0};
    const dim3 grid(plan.blocks), block(kSyncWaves * kSyncLanes);
    if (cfo) {
        DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_sc16_kernel<true>, plan.lds));
        hipLaunchKernelGGL(capture_sync_sc16_kernel<true>, grid, block, plan.lds, (hipStream_t)stream, args);
    } else {
        DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_sc16_kernel<false>, plan.lds));
        hipLaunchKernelGGL(capture_sync_sc16_kernel<false>, grid, block, plan.lds, (hipStream_t)stream, args);
    }
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_capture_sync_pooled_sc16(const int16_t* cap, long long n_samples, float scale, long long first, const long long* first_dev,
                                  long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                                  int32_t* offset, float* cfo_out, float* metric, void* workspace, size_t workspace_bytes,
                                  dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    // the pooled call's plan for one link; the link struct keeps its layout, its `cap` carries the address for the checks
    const dccn_pooled_link link{sc16_as_checked(cap), n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace,
                                workspace_bytes};
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(1, &link, frames, S, K, CP, W, out_kin, &plan, 4));
    DCCN_NO_CHAINS();
    plan.args.link[0].s.cap = nullptr;
    const PooledGroupArgs& g = plan.args;
    const PooledSc16Args args{g.link[0], CapSc16{cap, scale}, g.frames, g.S, g.K, g.CP, g.W, g.crop};
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_estimate_sc16_kernel, plan.lds_estimate));
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_cut_kernel<PooledSc16Args>, plan.lds_cut));
    const dim3 grid(plan.blocks, 1), block(kSyncWaves * kSyncLanes);
    hipLaunchKernelGGL(capture_pool_estimate_sc16_kernel, grid, block, plan.lds_estimate, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_reduce_kernel, dim3(1), dim3(kSyncLanes), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_cut_kernel<PooledSc16Args>, grid, block, plan.lds_cut, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_capture_acquire_sc16(const int16_t* cap, long long n_samples, float scale, long long lo, int J, int S, int K, int CP,
                              const int* pilot_sc, int n_pilot, long long* first_out, float* cfo_out, float* sym_metric,
                              float* phase_metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!sc16_scale_ok(scale)) return DCCN_ERR_INVALID_ARG;
    CaptureAcquirePlan plan;        // (the plan looks at sample counts and the base's alignment: nothing depends on the sample's size)
    DCCN_TRY(capture_acquire_plan(sc16_as_checked(cap), n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric,
                                  phase_metric, workspace, workspace_bytes, &plan));
    DCCN_NO_CHAINS();
    plan.args.cap = nullptr;
    const AcqSc16Args args{plan.args, CapSc16{cap, scale}};
    hipLaunchKernelGGL(acq_symbol_sums_sc16_kernel, dim3(plan.sum_blocks), dim3(kAcqSumThreads), 0, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_phase_sc16_kernel, dim3((unsigned)S, (unsigned)J), dim3(kAcqThreads), plan.lds, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_decide_kernel, dim3(1), dim3(kAcqMaxS), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- carrier offsets beyond half a subcarrier spacing: acquisition over (q, m), the cut with the whole offset taken out ---------
int dccn_capture_acquire_wide_supported(int S, int K, int CP, int n_pilot, int J, int M) {
    return capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M) ? 1 : 0;
}

size_t dccn_capture_acquire_wide_workspace_size(int S, int K, int CP, int n_pilot, int J, int M) {
    return capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M) ? capture_acquire_wide_layout(S, K, CP, J, M).total : 0;
}

int dccn_capture_acquire_wide(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                              int n_pilot, int M, long long* first_out, float* cfo_out, int32_t* cfo_int_out, float* sym_metric,
                              float* phase_metric, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!capture_acquire_wide_shape_ok(S, K, CP, n_pilot, J, M)) return DCCN_ERR_INVALID_ARG;
    if (!cfo_int_out || (reinterpret_cast<uintptr_t>(cfo_int_out) & 3u) != 0) return DCCN_ERR_INVALID_ARG;
    const AcqWorkspace w = capture_acquire_wide_layout(S, K, CP, J, M);
    // the narrow call's checks (the samples read are the same); its workspace is the M = 0 layout, a prefix of this one
    CaptureAcquirePlan plan;
    DCCN_TRY(capture_acquire_plan(cap, n_samples, lo, J, S, K, CP, pilot_sc, n_pilot, first_out, cfo_out, sym_metric, phase_metric,
                                  workspace, workspace_bytes, &plan));
    if (workspace_bytes < w.total) return DCCN_ERR_WORKSPACE;
    DCCN_NO_CHAINS();
    AcqWideArgs args{plan.args, cfo_int_out, M};
    args.a.rhat = reinterpret_cast<int*>(static_cast<char*>(workspace) + w.rhat);
    const size_t lds = capture_acquire_wide_lds(S, K, CP, n_pilot, M);
    DCCN_TRY(set_max_dynamic_smem((const void*)acq_phase_wide_kernel, lds));
    hipLaunchKernelGGL(acq_symbol_sums_kernel, dim3(plan.sum_blocks), dim3(kAcqSumThreads), 0, (hipStream_t)stream, args.a);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_phase_wide_kernel, dim3((unsigned)S, (unsigned)J), dim3(kAcqThreads), lds, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_decide_wide_kernel, dim3(1), dim3(kAcqWideThreads), 0, (hipStream_t)stream, args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

int dccn_capture_sync_wide(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                           int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                           float* metric, const int32_t* cfo_int_dev, const float* cfo_frac_dev, dccn_stream_t stream) {
    CaptureSyncPlan plan;
    DCCN_TRY(capture_sync_at_plan(cap, n_samples, first_dev, lo, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo, metric,
                                  &plan));
    if (!cfo || !wide_inputs_ok(cfo_int_dev, cfo_frac_dev)) return DCCN_ERR_INVALID_ARG;
    DCCN_NO_CHAINS();
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_sync_wide_kernel, plan.lds));
    hipLaunchKernelGGL(capture_sync_wide_kernel, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream,
                       CaptureSyncWideArgs{CaptureSyncAtArgs{plan.args, first_dev, lo}, CfoWide{cfo_int_dev, cfo_frac_dev}});
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

size_t dccn_capture_sync_pooled_wide_workspace_size(int frames) { return frames > 0 ? pooled_workspace_bytes(frames) + 16 : 0; }

int dccn_capture_sync_pooled_wide(const float* cap, long long n_samples, long long first, const long long* first_dev, long long lo,
                                  long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                                  int32_t* offset, float* cfo_out, float* metric, const int32_t* cfo_int_dev,
                                  const float* cfo_frac_dev, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    // the pooled call's plan with the fraction's slot (behind Gamma_f in the workspace) where it has cfo_out
    const size_t gamma_bytes = pooled_workspace_bytes(frames);
    const dccn_pooled_link link{cap, n_samples, first, first_dev, lo, stride, x_out, offset, cfo_out, metric, workspace, workspace_bytes};
    PooledGroupPlan plan;
    DCCN_TRY(pooled_group_plan(1, &link, frames, S, K, CP, W, out_kin, &plan));
    if (!wide_inputs_ok(cfo_int_dev, cfo_frac_dev)) return DCCN_ERR_INVALID_ARG;
    if (workspace_bytes < gamma_bytes + 16) return DCCN_ERR_WORKSPACE;
    DCCN_NO_CHAINS();
    plan.args.link[0].s.cfo = reinterpret_cast<float*>(static_cast<char*>(workspace) + gamma_bytes);
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_estimate_kernel, plan.lds_estimate));
    DCCN_TRY(set_max_dynamic_smem((const void*)capture_pool_cut_wide_kernel, plan.lds_cut));
    const dim3 grid(plan.blocks, 1), block(kSyncWaves * kSyncLanes);
    hipLaunchKernelGGL(capture_pool_estimate_kernel, grid, block, plan.lds_estimate, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_reduce_kernel, dim3(1), dim3(kSyncLanes), 0, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(capture_pool_cut_wide_kernel, grid, block, plan.lds_cut, (hipStream_t)stream,
                       PooledWideArgs{plan.args, CfoWide{cfo_int_dev, cfo_frac_dev}, cfo_out});
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

}  // extern "C"
