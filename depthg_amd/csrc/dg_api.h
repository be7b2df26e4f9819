// What the units of the C ABI share (dg_api_corr.hip, dg_api_head.hip, dg_api_eval.hip, dg_api_loss.hip, dg_api_data.hip, dg_api_aux.hip): error reporting and the
// library's second stream.  Internal: not installed beside include/depthg_corr.h.
#pragma once
#include "dg_common.h"

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <optional>

// ---- error reporting: one thread-local message for the whole library (dg_last_error), defined in dg_api_aux.hip
extern thread_local char g_err[512];
int fail(int code, const char* fmt, ...);
#define DG_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(DG_ERR_LAUNCH, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

static inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- the argument checks the entry points with a workspace share (dg_api_loss.hip, the depth encoder of dg_api_aux.hip, the augmentation of dg_api_data.hip)
// the pointers of `p4` on 4-byte boundaries (a null optional pointer passes), the workspace on a 16-byte one
inline int check_aligned(const char* who, std::initializer_list<const void*> p4, const void* workspace) {
    uintptr_t bits = 0;
    for (const void* p : p4) bits |= (uintptr_t)p;
    if ((bits & 3) || ((uintptr_t)workspace & 15))
        return fail(DG_ERR_INVALID, "%s: the tensors must be 4-byte aligned, workspace 16-byte aligned", who);
    return DG_OK;
}

inline int check_workspace(const char* who, size_t workspace_bytes, size_t need, const char* sizer) {
    if (workspace_bytes < need) return fail(DG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", who, workspace_bytes, need, sizer);
    return DG_OK;
}

// A second stream of the library's own (one per device, created on the first call that is not being captured into a graph) for the
// launches that may run beside each other inside one call; null while none exists and the caller's stream is capturing (creating
// one there is not a capturable operation: the call then launches in sequence).
struct SideStream { hipStream_t s; hipEvent_t fork, join, mid[2]; std::mutex use; };
SideStream* side_stream_for(hipStream_t caller);        // (dg_api_aux.hip)

// One fork .. join region on the device's side stream.  The stream and its event pair are shared by every caller on the device, so
// the region holds the stream's lock from the fork record to the join wait: two host threads (or two caller streams) cannot interleave
// their records and waits.  Whatever happens after the fork - a failed launch returns through DG_HIP - the destructor still records
// the join and makes the caller's stream wait for it: the side stream is never left unjoined (inside a hipGraph capture that would be
// a forked capture that cannot end).
struct SideRegion {
    SideStream* side;
    hipStream_t caller;
    std::unique_lock<std::mutex> lk;
    bool forked = false, join_recorded = false, joined = false;
    explicit SideRegion(hipStream_t caller_) : side(side_stream_for(caller_)), caller(caller_) {
        if (side) lk = std::unique_lock<std::mutex>(side->use);
    }
    explicit operator bool() const { return side != nullptr; }
    hipStream_t stream() const { return side->s; }
    hipError_t fork() {
        hipError_t e = hipEventRecord(side->fork, caller);
        if (e != hipSuccess) return e;
        e = hipStreamWaitEvent(side->s, side->fork, 0);
        forked = e == hipSuccess;
        return e;
    }
    void reset() { forked = join_recorded = joined = false; }         // (after a join: the region may fork again)
    hipError_t record_join() {
        hipError_t e = hipEventRecord(side->join, side->s);
        join_recorded = e == hipSuccess;
        return e;
    }
    // hand-over i in mid-region: everything launched on the side stream so far is ordered in front of what the caller launches next
    hipError_t hand_over(int i) {
        hipError_t e = hipEventRecord(side->mid[i], side->s);
        if (e != hipSuccess) return e;
        return hipStreamWaitEvent(caller, side->mid[i], 0);
    }
    hipError_t join() {
        if (!forked || joined) return hipSuccess;
        if (!join_recorded) { hipError_t e = record_join(); if (e != hipSuccess) return e; }
        hipError_t e = hipStreamWaitEvent(caller, side->join, 0);
        joined = e == hipSuccess;
        return e;
    }
    ~SideRegion() { if (side && forked && !joined) (void)join(); }
};
