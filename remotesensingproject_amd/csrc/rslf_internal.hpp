// What the translation units of librslf_hip.so share: the error convention and the exception barrier of the C-ABI, the
// context / volume / multi-device objects, and the helpers one unit offers the others.  No kernels here -- each unit
// includes the kernel headers it launches (device code is per translation unit).
//
//   rslf_core.hip         errors, contexts, volumes, host upload / device pack (K0)
//   rslf_pile.hip         the hot path: edge confidence (K1), scan (K2), selective median (K3), Depth1DComputer(_pile)
//   rslf_chip_a/b/c.hip   the on-chip scan kernel's instantiations, one per rung of its ladder (launched by rslf_pile.hip)
//   rslf_scores.hip       the scan's score matrix as an output: rslf_depth_epi_scores and its host form (k2_scores.hpp)
//   rslf_peaks.hip        the score rows' consumer: winner, sub-grid disparity and runner-up per pixel (k8_peaks.hpp)
//   rslf_subgrid.hip      the arg max moved off the grid: the winner's two neighbours re-scored, no row in memory (k9_subgrid.hpp)
//   rslf_sweep_peaks.hip  the 2-D sweep's peaks mode: winner and runner-up of a visit's scanned pixels, no row kept (k10_sweep_peaks.hpp)
//   rslf_sweep.hip        the 2-D sweep and its propagation (K4), Depth2DComputer::run
//   rslf_f2c.hip          fine-to-coarse: pyramid, bound tightening, fusion (K5) and the one native level loop
//   rslf_f2c_keep.hip     a finished fine-to-coarse run kept on the device (rslf_f2c_run): copies out, the coloured getters
//   rslf_f2c_peaks.hip    a kept run's peak planes: validity by uniqueness and the fused peaks (k11_f2c_peaks.hpp)
//   rslf_render.hip       the getters' pictures: fit, plane render, EPI line painter (K6)
//   rslf_consistency.hip  cross-view consistency of a sweep's disparity planes: counts, fused value, validity (k12_consistency.hpp),
//                         and its gate form for a kept fine-to-coarse run's levels (k13_f2c_consistency.hpp)
//   rslf_warp.hip         the view warp: any view position from a sweep's planes, z-buffered (k14_view_warp.hpp)
//   rslf_novel.hip        the novel view: the warp's holes filled, the views that see a point blended (k15_novel_view.hpp)
//   rslf_stack_op.hpp     the host frame of those three units' four forms each (device planes, host planes, a kept run, a kept run
//                         with host outputs): a kept run's plane pair, the open-sweep refusal, the staging of host inputs and
//                         outputs (layout: rslf_plan_stage.hpp), and the checks and launch batches the warp and the novel view share
//   rslf_dilate.hip       the dilation along u: a volume f times as wide by a good kernel, result planes back (k16_dilate.hpp)
//   rslf_equalize.hip     the per-view equalisation: a view's quantised statistics, (a, b) per view and channel, y = a x + b (k19_equalize.hpp)
//   rslf_derivative.hip   the derivative channels: a one-channel field as (x, |dx/du|, |dx/dv|), volume and raw level (k17_derivative.hpp)
//   rslf_multi.hip        host pointers in / host planes out, pipelined over one or several devices (pile path)
//   rslf_multi_sweep.hip  the 2-D sweep sharded over several devices, and fine-to-coarse with its levels swept so
//   rslf_plan.hpp         every host-side decision as pure functions (unit-tested on the CPU under ASan / UBSan)
//   rslf_plan_peaks.hpp, rslf_plan_render.hpp, rslf_plan_subgrid.hpp, rslf_plan_sweep_gate.hpp, rslf_plan_consistency.hpp, rslf_plan_warp.hpp, rslf_plan_dilate.hpp, rslf_plan_derivative.hpp   ... continued, for the units that need them
//   rslf_scratch.hpp      GrowBuf, the one owning buffer type (host-only, unit-tested likewise); its allocators are below
//
// Two rules of the multi-device paths: they never write into a rslf_volume they did not create (a chunk of another height
// is a local non-owning copy of the volume object, rslf_multi.hip's Worker::view), and a context's stream is changed only
// through StreamScope (below), which puts it back when its scope ends.
#pragma once

#include "../../include/rslf_hip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "rslf_device.hpp"
#include "rslf_plan.hpp"
#include "rslf_scratch.hpp"

// ---- errors ---------------------------------------------------------------

namespace rslf {

char* last_error_buffer();   // thread-local, 512 bytes (rslf_core.hip)

inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// Testing hook (rslf_debug_inject, include/rslf_hip.h): the named site throws / fails the next `count` times it is
// reached.  One relaxed atomic load per site visit; sites sit on host control paths only, never in a launch loop.
enum InjectSite { kInjectWorker = 0, kInjectThreadCreate = 1, kInjectAlloc = 2, kInjectSweep = 3, kInjectSites = 4 };
bool inject_hit(InjectSite site);   // true (and one count consumed) when the site should fail now

}  // namespace rslf

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return rslf::fail(RSLF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The exception barrier of the C boundary (include/rslf_hip.h: "never throws across the boundary"; the reference's seam
// returns void and has no error path at all, core.hpp:279-310).  EVERY `extern "C" int rslf_*` definition is a
// function-try-block closed by this handler list -- tests/test_abi.py greps for it:
//
//     extern "C" int rslf_foo(args) RSLF_API_TRY
//     {
//         ...
//     }
//     RSLF_API_CATCH
//
// std::bad_alloc -> RSLF_ERR_ALLOC, any other std::exception -> RSLF_ERR_INTERNAL with its what() in rslf_last_error(),
// anything else -> RSLF_ERR_INTERNAL.  Threads started inside an entry point are owned by a JoinGuard, so an exception (or
// an early return) can never leave a joinable std::thread behind (std::terminate).
#define RSLF_API_TRY try
#define RSLF_API_CATCH                                                                              \
    catch (const std::bad_alloc&)                                                                   \
    {                                                                                               \
        return rslf::fail(RSLF_ERR_ALLOC, "out of host memory (std::bad_alloc)");                   \
    }                                                                                               \
    catch (const std::exception& e_)                                                                \
    {                                                                                               \
        return rslf::fail(RSLF_ERR_INTERNAL, "internal error: %s", e_.what());                      \
    }                                                                                               \
    catch (...)                                                                                     \
    {                                                                                               \
        return rslf::fail(RSLF_ERR_INTERNAL, "internal error: unknown exception");                  \
    }

namespace rslf {

// Owns the worker threads of one entry point: joins whatever is joinable when the scope ends, however it ends.
// run(f): on a new thread if one can be had, else on the calling thread (std::system_error from the constructor -- the
// GPU boxes cap a process's threads -- or an injected failure) -- the work is done either way.
class JoinGuard {
public:
    JoinGuard() = default;
    JoinGuard(const JoinGuard&) = delete;
    JoinGuard& operator=(const JoinGuard&) = delete;
    ~JoinGuard() { join_all(); }
    template <typename F>
    void run(F f)
    {
        bool started = false;
        try {
            if (!inject_hit(kInjectThreadCreate)) {
                threads_.reserve(threads_.size() + 1);   // may throw bad_alloc: before the thread exists
                threads_.emplace_back(f);
                started = true;
            }
        } catch (const std::system_error&) {
            started = false;
        }
        if (!started)
            f();   // no thread to be had: the caller does the work itself
    }
    void join_all()
    {
        for (std::thread& t : threads_)
            if (t.joinable())
                t.join();
        threads_.clear();
    }

private:
    std::vector<std::thread> threads_;
};

// Runs `f` (an `int()` returning an rslf status) and turns anything it throws into a status + message, for worker threads:
// an exception must not leave a thread function either.
template <typename F>
int guarded_status(F f, std::string* err)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        if (err)
            *err = "out of host memory (std::bad_alloc)";
        return RSLF_ERR_ALLOC;
    } catch (const std::exception& e) {
        if (err)
            *err = std::string("internal error: ") + e.what();
        return RSLF_ERR_INTERNAL;
    } catch (...) {
        if (err)
            *err = "internal error: unknown exception";
        return RSLF_ERR_INTERNAL;
    }
}

}  // namespace rslf

// ---- objects --------------------------------------------------------------

namespace rslf {

// The allocators of GrowBuf (rslf_scratch.hpp): device memory and pinned host memory.  Their frees wait for the device's
// outstanding work; no other code of the library frees (a volume's slab apart, rslf_volume_destroy).
struct DeviceAlloc {
    static int alloc(size_t bytes, void** out) { return (int)hipMalloc(out, bytes); }
    static int free(void* p) { return (int)hipFree(p); }
};
struct PinnedAlloc {
    static int alloc(size_t bytes, void** out) { return (int)hipHostMalloc(out, bytes, hipHostMallocDefault); }
    static int free(void* p) { return (int)hipHostFree(p); }
};
using DeviceBuf = GrowBuf<DeviceAlloc>;
using PinnedBuf = GrowBuf<PinnedAlloc>;

// The one error convention of a regrow: HIP_TRY(hip_err(buf.reserve(bytes))) -- a failed free or allocation is RSLF_ERR_HIP
// with HIP_TRY's message.
inline hipError_t hip_err(Reserved r) { return (hipError_t)r.err; }

// The buffers that several entry points share (Scratch::shared, handed out by helper_scratch): the once-per-level helpers of
// fine-to-coarse and the renderers, whose largest users are as large as a pyramid level -- sharing them is what keeps a
// context's footprint at one set.  Sharing is safe because every entry point queues all its work on the context's stream,
// in order, and none keeps a pointer to a shared buffer past its return: the next user's launches run after the previous
// user's.  (A buffer that IS held across calls -- the line-confidence columns of an open sweep -- is a member of its own.)
enum SharedBuf {
    kSharedLevel = 0,    // rslf_downsample_epis_*: the row pass over a whole raw level [V][S][U][C]; rslf_f2c_fuse: running map A
    kSharedTable,        // rslf_f2c_fuse: running mask A; the renderers: colour table and the planes' (a, b) (upload_table)
    kSharedLeft,         // rslf_f2c_tighten_bounds: nearest valid pixel to the left, [S][V][U] ints; rslf_f2c_fuse: running map B; the renderers' fit: its state
    kSharedRight,        // rslf_f2c_tighten_bounds: ... to the right; rslf_f2c_fuse: running mask B; the fit: its slab
    kSharedStagePlanes,  // the renderers' host-pointer forms: the planes / the depth rows on the device,
    kSharedStageMask,    // ... their validity / mask bytes,
    kSharedStageOut,     // ... and the pictures before they go back
    kSharedBufs
};

// Every piece of device memory a context owns.  Each buffer has a capacity of its own (a capacity shared by buffers of
// different shapes once let a later volume overrun the smaller one: tools/fuzz_sweep.py), grows on demand -- never inside a
// timed launch sequence after the first call -- and is freed by its destructor.
struct Scratch {
    DeviceBuf total;        // 2 x u64, made with the context: [0] scanned pixels, [1] the packed list's length (packed_len)
    DeviceBuf minmax;       // float [2], made with the context: a volume's value range while it is packed
    DeviceBuf list;         // int [V*U]: the pixels a scan visits, per scanline or as one packed list
    DeviceBuf depth_tmp;    // float [V*U]: the raw disparities of a pile step; a byte plane for the opening (morph_tmp)
    DeviceBuf count;        // int [V]: pixels per scanline
    DeviceBuf rowbase;      // int [V]: where each scanline's pixels start in the packed list
    DeviceBuf partial;      // float [rows][2]: min / max partials of the pack kernels
    DeviceBuf staging;      // host uploads pass through here in chunks
    DeviceBuf scan_partial; // rslf::Partial [tile][group][64]: records of grouped scan launches
    DeviceBuf scan_ticket;  // int [tile] of the same launches: which group merges the tile (zero between launches)
    DeviceBuf max_partial;  // float [kMaxPartials]: block maxima of rslf_device_max_f32
    DeviceBuf sub_idx;      // int32 [V*U]: a sub-grid pile step's arg-max plane when the caller passes none (subgrid_planes); a sub-grid sweep's visits' (rslf_sweep_subgrid)
    DeviceBuf sub_score;    // float [V*U]: ... and their score plane
    DeviceBuf pk_list;      // int [V*U]: per-scanline pixel lists of a peaks sweep's dense step (rslf_sweep_peaks) -- its own: `list` is the scans'
    DeviceBuf pk_count;     // int [V] + one u64: ... their counts and pixel total (plan::sweep_peaks_count_bytes)
    DeviceBuf pk_mask;      // u8 [V*U]: ... and the step's mask, "this visit's idx >= 0"
    DeviceBuf row_exact;    // the scan's row-exact table (k2_scan.hpp, ScanArgs::rx_*): [D][slots] offsets, [D][slots] weight pairs, [D] floats, [D] ints; RowExactKey says of what
    // 2-D sweep
    DeviceBuf winner;       // int [S][V][U]: the claims (0x7F7F7F7F between visits)
    DeviceBuf sweep_mask;   // u8 [S][V][U]: the running masks, unless the caller gives the plane
    DeviceBuf dirty;        // u8 [S][V][ceil(U/256)]: segments of the winner rows that hold a claim (all 0 between visits)
    DeviceBuf remain;       // int [S][V][ceil(U/256)]: pixels left in the running mask per segment (lets the claims skip views)
    DeviceBuf filtered;     // float [V][U]: median of the visited view, the propagation's source
    DeviceBuf withheld;     // one u64: sources a gated sweep withheld (rslf_sweep_propagation_ratio zeroes it, the claims count, rslf_sweep_withheld reads)
    DeviceBuf lc_columns;   // float [V][S][U]: K(r - rbar) columns of a sweep with line confidence, kept from visit to visit
    DeviceBuf lc_argmax;    // int32 [V][U]: arg-max indices of the visit's scan, -1 where it accepted nothing
    // per-view equalisation (K19)
    DeviceBuf eq_stats;     // u64 [S][C][3]: a view's (n, s1, s2) per channel, zeroed on the context's stream before every count
    DeviceBuf eq_table;     // float [S][C][2]: the (a, b) the apply kernel reads, copied from rslf_ctx::eq_table_host
    DeviceBuf shared[kSharedBufs];

    static constexpr size_t kMaxPartials = 2048;
    unsigned long long* pixel_total() const { return total.as<unsigned long long>(); }
    int* packed_len() const { return reinterpret_cast<int*>(pixel_total() + 1); }   // an int in the second u64 of `total`
    uint8_t* morph_tmp() const { return depth_tmp.as<uint8_t>(); }                   // V*U floats: room for a byte plane
};

// Slots per hypothesis of the row-exact table a register row kernel of `spad` slots x C channels reads, 0: the kernel has no
// scalar-tap form (k2_reg.hpp, scan_reg_scalar_taps: the 104-slot one-channel kernel) -- and the table's size in bytes:
// [dim_d][slots] 8-byte offsets, [dim_d][slots] weight pairs, [dim_d] disparities, [dim_d] flags.
constexpr int row_exact_slots(int spad, int C) { return (C == 1 && spad == 104) ? spad : 0; }
constexpr size_t row_exact_bytes(int dim_d, int slots) { return (size_t)dim_d * ((size_t)slots * 16 + 8); }

// What the row-exact table in Scratch::row_exact was made from: everything its entries depend on.  A scan with the same key
// finds the table in place (a pile call after another, the frames of a sequence); any other key refills it on the scan's
// stream, ahead of the scan -- so does each visit of a 2-D sweep that takes the row kernel: the entries depend on s_hat.
struct RowExactKey {
    float dmin = 0.0f, dmax = 0.0f, slope = 0.0f;
    int dim_d = 0, s_hat = 0, S = 0, U = 0, C = 0, slots = 0;   // dim_d == 0: no table yet
    long long stride_s = 0;
    const void* queued_on = nullptr;   // the stream the fill was queued on: a scan on another one is not ordered after it, and refills
    bool same(const RowExactKey& o) const
    {
        // (floats by their bits: a NaN key never matches, -0 and +0 differ)
        return memcmp(&dmin, &o.dmin, sizeof(float)) == 0 && memcmp(&dmax, &o.dmax, sizeof(float)) == 0 &&
               memcmp(&slope, &o.slope, sizeof(float)) == 0 && dim_d == o.dim_d && s_hat == o.s_hat && S == o.S && U == o.U && C == o.C &&
               slots == o.slots && stride_s == o.stride_s && queued_on == o.queued_on;
    }
};

// An open 2-D sweep (rslf_sweep_begin .. rslf_sweep_end).  The defaults are "no sweep open": sweep_close assigns them.
struct SweepState {
    bool open = false;          // between rslf_sweep_begin and rslf_sweep_end
    bool keep_total = false;    // the sweep sums the scanned pixels of all its visits
    bool first = true;          // the next visit is the sweep's first (dense) one; true outside a sweep: scan_defaults times every scan then
    bool scanned = false;       // a visit of the open sweep has scanned (rslf_sweep_line_confidence comes before)
    bool listed = false;        // the last apply pass listed the next visit's pixels (packed list and length in place); else k34_median_claim left the list's length at 0
    int expect = -1;            // the view the sweep visits next (core.hpp:981-990), -1 once all are done
    uint8_t* mask_run = nullptr;   // the running masks [S][V][U]
    // line confidence (rslf_sweep_line_confidence; k7_line_conf.hpp): state of ONE sweep.  The K columns and the visit's
    // arg-max plane are Scratch::lc_columns / lc_argmax, sized when the mode is set, never inside a visit.
    int lc_mode = RSLF_LINE_CONF_OFF;
    float* lc_Cl_svu = nullptr;        // the caller's [S][V][U] plane
    float* lc_K_vsu = nullptr;         // (core.hpp:975-979)
    int32_t* lc_idx_vu = nullptr;
    // what rslf_sweep_visit_scan was given and K7 needs to re-run a winning hypothesis (rslf_sweep_visit_finish is not told)
    const float* lc_Ce_svu = nullptr;
    const float* lc_dmin_vu = nullptr;
    const float* lc_dmax_vu = nullptr;
    float lc_dmin = 0.0f, lc_dmax = 0.0f;
    int lc_dim_d = 0;
    ScanConsts lc_consts = {};
    // sub-grid mode (rslf_sweep_subgrid; k9_subgrid.hpp): state of ONE sweep too.  The visit's arg-max and score planes are
    // Scratch::sub_idx / sub_score, sized when the mode is set; with line confidence on, the arg-max plane is K7's
    // (Scratch::lc_argmax): one plane for both.
    bool subgrid = false;
    // peaks mode (rslf_sweep_peaks; k10_sweep_peaks.hpp): state of ONE sweep too.  The caller's four [S][V][U] planes (disp
    // stays NULL); the visits' arg-max plane is the one above, the dense step's lists Scratch::pk_*.
    bool peaks = false;
    rslf_peaks pk = {};
    int dim_d = 0;              // what rslf_sweep_begin was given: sizes the dense step's staging when the mode is set
    // gate by peak ratio (rslf_sweep_propagation_ratio; k4_propagate.hpp): state of ONE sweep too, 0 = off.  Needs the peaks
    // mode with all four planes; its counter is Scratch::withheld.
    float prop_ratio = 0.0f;
};

}  // namespace rslf

struct rslf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    rslf::Scratch scratch;
    rslf::SweepState sweep;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    // "time_all" (rslf_ctx_set_debug): every scan launch sequence is bracketed by its own pair of events from this pool --
    // rslf_scan_time_total_ms sums them -- so that a sweep's or a pyramid's SUMMED K2 time can be reported (bench.py's
    // roofline on the sweep2d / f2c lines).  Off by default: an event is a packet of its own in the queue (~5.6 us each).
    int time_all = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    int last_spad = 0;   // register-scan slot count of the last K2 launch, 0 = none
    int last_kernel = 0; // RSLF_SCAN_* of the last K2 launch
    bool last_gated = false;   // the last sweep that ended well had the ratio set: Scratch::withheld holds its count (rslf_sweep_withheld)
    int num_cus = 0;           // compute units of the device (how many workgroups a launch needs to fill it)
    // test / tuning hooks (rslf_ctx_set_debug), per context: 0 / -1 = automatic
    int force_scan = 0;        // 1 generic kernel, 2 streaming kernel wherever it can run (never the on-chip one)
    int force_groups = 0;      // hypothesis groups per tile
    int force_packed = -1;     // 0 / 1
    int px_mode = -1;          // pixel-per-wave kernel on packed launches: -1 automatic, 0 never, 1 whenever it can run
    int stream_groups = 0;     // streaming kernel, dense launches: hypothesis groups per tile (0 = kStreamGroups)
    int stream_share = 1;      // streaming kernel: 63-pixel row tiles whose tail shares taps between neighbouring lanes: 0 never, 1 where the tail is long (plan::stream_shares_taps), 2 always
    size_t stream_lds_bytes = rslf::plan::kStreamLdsBytes;   // dynamic LDS of one streaming workgroup
    int row_split = 1;         // packed launches of stream-class volumes: rows with many pixels as row tiles of the list (0: off; A/B and tests)
    int tap_table = 1;         // register row kernels that have one take lane-invariant lerp taps from it (k2_reg.hpp; 0: off, A/B and tests)
    int scalar_taps = 1;       // ... and row-exact hypotheses take the scalar-tap form from the per-launch table (k2_reg.hpp; 0: off, A/B and tests)
    rslf::RowExactKey row_exact_key;   // what scratch.row_exact holds
    bool last_row_exact = false;       // the last scan's launch was handed the table (rslf_last_scan_row_exact)
    int subgrid_list = 1;      // 2-D sweep in the sub-grid mode: sparse visits refine over the packed list (0: every visit the dense form; A/B and tests)
    int peaks_list = 1;        // 2-D sweep in the peaks mode: sparse visits take k10_peaks_list over the packed list (0: every visit the dense form; A/B and tests)
    int claim_skip = 1;        // 2-D sweep: the claims skip views with nothing left to paint within reach (0: off, A/B and tests)
    int staging_kib = 0;       // chunked host upload: device staging per pass in KiB (0: plan::kStagingBudget; tests of the later passes)
    std::vector<float> eq_table_host;   // K19: the host copy of scratch.eq_table: outlives the copy that reads it
    int consistency_order = 0; // K12: the grid's order (k12_consistency.hpp, ConsistencyOrder; 0: scanlines dealt to the XCDs; A/B and tests)
};

struct rslf_volume {
    rslf_ctx* ctx = nullptr;
    int device = 0;   // kept here too: a volume may be destroyed after its context
    int V = 0, S = 0, U = 0, C = 0, pitch = 0;
    float* base = nullptr;
    size_t bytes = 0;
    float min_value = 0.0f, max_value = 0.0f;
    bool filled = false;
};

struct rslf_multi {
    struct Dev {
        rslf_ctx* ctx = nullptr;
        hipStream_t s_up = nullptr, s_comp = nullptr, s_down = nullptr;
        hipEvent_t done[2] = {nullptr, nullptr};
        rslf_volume* vol[2] = {nullptr, nullptr};   // as tall as the tallest chunk so far; never written once made
        rslf::DeviceBuf planes[2];           // result planes of the chunk being computed and of the one being collected
        rslf::PinnedBuf pin[2];              // pinned host staging for EPIs scattered over the heap (Vec<Mat>)
        rslf::DeviceBuf arena;               // the sweep forms' planes, kept from call to call (and from level to level)
    };
    std::vector<Dev> devs;
    int chunk_rows = 0;   // 0 = automatic
    // peer access between the devices of this object (rslf_multi_create): peer[i * n + k] = device i can map device k's
    // memory (hipDeviceCanAccessPeer) AND the access is enabled; copies between devices without it stage through the host
    std::vector<unsigned char> peer;
};

namespace rslf {

// The one way the library changes a context's stream (rslf_ctx_set_stream is the caller's): for a scope, put back when it
// ends, however it ends.
struct StreamScope {
    StreamScope(rslf_ctx* ctx_, hipStream_t stream) : ctx(ctx_), saved(ctx_->stream) { ctx->stream = stream; }
    ~StreamScope() { ctx->stream = saved; }
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
    rslf_ctx* const ctx;
    const hipStream_t saved;
};

inline VolView view_of(const rslf_volume* vol)
{
    VolView w;
    w.base = vol->base;
    w.V = vol->V;
    w.S = vol->S;
    w.U = vol->U;
    w.C = vol->C;
    w.pitch = vol->pitch;
    w.stride_s = (long long)vol->pitch * vol->C;
    w.stride_v = (long long)vol->S * w.stride_s;
    return w;
}

inline float scale_of(float epi_scale_factor)
{
    return (float)(1.0 / (double)epi_scale_factor);   // dc.hpp:474 through cvtScale's float scale
}

// scoped device memory of the once-per-call helpers: the same owning type, allocated once.  A 0-byte request becomes a
// 1-byte one, so an empty plane still has an address.
struct DevBuf : DeviceBuf {
    hipError_t alloc(size_t bytes) { return hip_err(reserve(bytes ? bytes : 1)); }
};

// rslf_core.hip
int check_params(const rslf_params* p);
ScanConsts make_scan_consts(const rslf_params* p);
int ensure_plane_scratch(rslf_ctx* ctx, int V, int U);
int ensure_group_scratch(rslf_ctx* ctx, size_t recs, size_t tiles, bool* tickets_fresh = nullptr);
int ensure_staging(rslf_ctx* ctx, size_t bytes);
int helper_scratch(rslf_ctx* ctx, SharedBuf which, size_t bytes, void** out);
// the range of a volume from n (min, max) pairs a kernel left in the pack kernels' partials (rslf_derivative.hip)
int range_partials(rslf_ctx* ctx, size_t n, float** out);
int volume_range_from_partials(rslf_volume* vol, int n);
// The element type of a host light field (the cv::Mat depths the reference's constructors take, dc.hpp:269-288,
// :442-475, :671-705): CV_32F, CV_8U, CV_16U.  Chosen once at the C-ABI entry point; everything below it dispatches on it.
enum class Elem { F32, U8, U16 };
inline size_t elem_bytes(Elem e) { return e == Elem::F32 ? sizeof(float) : e == Elem::U8 ? 1 : sizeof(uint16_t); }
// dc.hpp:442-460 over host rows: max(start, every value as float) -- exact for ushort, so a u16 field's max equals the
// max of the same values given as float
template <typename T>
float host_max(const T* const* h_ptrs, int n_ptrs, int rows, size_t row_stride_bytes, size_t row_elems, float start);
template <typename T>
float host_max_parallel(const T* const* h_epis, int V, int S, size_t stride, size_t row_elems, float start);
// The constructor's epi_scale_factor for element type e: CV_8U -> 255 (the factor is ignored, dc.hpp:470); every other
// depth -> the given factor, or when it is < 0 the max over every value of the n_ptrs x rows host rows (dc.hpp:442-475).
// The stored value is then x * scale_of(factor) for every type (scale_of(255) == float(1/255)).
float resolve_scale_factor(Elem e, const void* const* h_ptrs, int n_ptrs, int rows, size_t row_stride_bytes, size_t row_elems,
                           float epi_scale_factor, bool parallel);
template <typename SrcT>
int upload_host(rslf_volume* vol, const SrcT* const* h_ptrs, size_t row_stride_bytes, bool image_major, float scale);
extern template int upload_host<float>(rslf_volume*, const float* const*, size_t, bool, float);
extern template int upload_host<uint8_t>(rslf_volume*, const uint8_t* const*, size_t, bool, float);
extern template int upload_host<uint16_t>(rslf_volume*, const uint16_t* const*, size_t, bool, float);
// upload_host for a field of element type e
int upload_host_elem(rslf_volume* vol, Elem e, const void* const* h_ptrs, size_t row_stride_bytes, bool image_major, float scale);

// rslf_pile.hip
// What a scan is given besides the arguments of rslf_depth_epi_scan: where its pixel lists come from and the launch shape
// its caller asks for.  The public entry points pass scan_defaults.
struct ScanInputs {
    enum Lists { kCompact = 0, kRowLists = 1, kPackedList = 2 };   // (plan::ScanRequest::precompacted)
    int lists = kCompact;         // the scan compacts the mask / K1 left per-row lists and the total / a sweep's apply pass
                                  // left the packed list and its length
    int groups = 1;               // hypothesis groups per tile (a sweep's sparse visits ask for more)
    bool packed = false;          // one packed pixel list over all scanlines
    bool packed_n_zero = false;   // the packed list's length is already 0
    bool zero_total = true;       // the pixel total starts again
    bool timed = true;            // ctx->ev0 / ev1 bracket the launches (rslf_last_scan_kernel_ms)
    bool clear_score = true;      // a score plane starts at 0 (a sweep's sub-grid visits read it only where this scan wrote idx: no fill)
};
ScanInputs scan_defaults(const rslf_ctx* ctx);
int depth_epi_scan(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                   int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu,
                   const rslf_params* p, uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats,
                   const ScanInputs& in);
// The arguments every scan of the hypothesis grid takes (K2, the K columns, the sub-grid refinement)
int check_scan_args(const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, int dim_d, int s_hat, const rslf_params* p);
void fill_stats(rslf_ctx* ctx, unsigned long long tot, int dim_d, rslf_stats* stats);
int read_stats(rslf_ctx* ctx, int dim_d, rslf_stats* stats);
int scan_presize(rslf_ctx* ctx, int S, int U, int C, int dim_d, const rslf_params* p, const int* rows, int n_rows);
int sweep_scan_presize(rslf_ctx* ctx, const rslf_volume* vol, int dim_d, const ScanInputs& sparse);

// rslf_scores.hip
// What rslf_depth_epi_scores checks before anything is queued (`out`: the caller's output, non-NULL), and the rows of the
// scanlines [v_first, v_first + n_rows) into d_scores ([n_rows][U][dim_d]) with arguments already checked: queued on the
// context's stream, the scanned pixels left in scratch.pixel_total().  read_pixel_total waits for the stream.
int check_score_args(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, int dim_d, int s_hat,
                     const rslf_params* p, int v_first, int n_rows, const void* out);
// own (nullable): pixel lists [V][U], counts [V] and a pixel total that are not the context's -- a peaks sweep's dense step,
// inside an open sweep whose lists and total are in use (rslf_sweep_peaks.hip).
struct ScoreLists {
    int* list;
    int* count;
    unsigned long long* total;
};
int score_rows(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax, int dim_d,
               int s_hat, const rslf_params* p, const uint8_t* d_mask_vu, int v_first, int n_rows, float* d_scores, int* kind_out,
               int* spad_out, const ScoreLists* own = nullptr);
int read_pixel_total(rslf_ctx* ctx, unsigned long long* tot);
void score_stats(unsigned long long pixels, int dim_d, int kind, int spad, rslf_stats* stats);

// rslf_peaks.hip
// k8_score_peaks over the pixels of scanlines [v_first, v_first + n_rows) of [V][U] planes (`out`: that window's planes);
// arguments checked, one launch queued on the context's stream.
int launch_score_peaks(rslf_ctx* ctx, const float* d_scores, int U, int dim_d, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                       float dmax, const uint8_t* d_mask_vu, int v_first, int n_rows, const rslf_peaks& out);

// rslf_sweep_peaks.hip
// The peaks step of a visit of an open sweep in the mode (rslf_sweep_peaks), queued after the scan: form is a
// plan::PeaksForm (0: nothing).  idx_vu: the visit's arg-max plane.  Writes the visited view's planes of ctx->sweep.pk.
int sweep_peaks_step(rslf_ctx* ctx, const rslf_volume* vol, const float* dmin_vu, const float* dmax_vu, float dmin, float dmax,
                     int dim_d, int s_hat, const rslf_params* p, const int32_t* idx_vu, int form);

// rslf_subgrid.hip
// k9_subgrid_refine over a volume's [V][U] planes, arguments already checked (check_scan_args): one launch queued on the
// context's stream.  d_score_vu, d_left_vu, d_right_vu nullable; d_disp_vu may be the scan's depth plane.  listed: lane =
// entry of the context's packed list (k9_subgrid_refine_list), for a sweep's visit whose scan took that list.
int subgrid_refine(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                   int dim_d, int s_hat, const rslf_params* p, const int32_t* d_idx_vu, const float* d_score_vu, float* d_disp_vu,
                   float* d_left_vu, float* d_right_vu, bool listed = false);

// rslf_sweep.hip
// Depth2DComputer::run (dc.hpp:748-805) on device planes; d_dmin_svu / d_dmax_svu: per-pixel ranges (a fine-to-coarse
// level, dc.hpp:201-203), or both NULL for the scalar range.
// The six [S][V][U] result planes of a sweep, which always travel together (rbar has C floats per pixel; scan_mask nullable).
struct SweepPlanes {
    float* Ce = nullptr;
    uint8_t* Ce_mask = nullptr;
    float* Cd = nullptr;
    float* depth = nullptr;
    float* rbar = nullptr;
    uint8_t* scan_mask = nullptr;
};
// What a sweep is asked for beyond the reference's arguments; the defaults are the reference's sweep, and every mode left at
// its default queues exactly the launches of the sweep without it.
struct SweepModes {
    int line_mode = RSLF_LINE_CONF_OFF;   // RSLF_LINE_CONF_* (dc.hpp:721-738, :791-792) ...
    float* Cl_svu = nullptr;              // ... and its [S][V][U] plane, zero-filled by depth2d_run; NULL when off
    int subgrid = 0;                      // 1: every visit in the sub-grid mode (rslf_sweep_subgrid)
    const rslf_peaks* peaks = nullptr;    // the peaks mode's four planes (rslf_sweep_peaks), filled by depth2d_run with
                                          // idx = runner_idx = -1 and the floats 0; NULL: mode off
    float propagation_ratio = 0.0f;       // > 0: the sweep gated by it (rslf_sweep_propagation_ratio); needs the four planes
};
// The one place a sweep's modes are checked: the gate, the line mode, its plane, subgrid.  Every entry runs it once, before
// anything is allocated or queued.
int check_sweep_modes(const SweepModes& modes);
int depth2d_run(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin, float dmax,
                int dim_d, const rslf_params* p, const SweepPlanes& d_out, rslf_stats* stats, const SweepModes& modes);

// rslf_f2c.hip
// A volume owned by a scope or an object (rslf_volume_destroy is the one place that frees a slab).
struct VolumeDeleter {
    void operator()(rslf_volume* vol) const { rslf_volume_destroy(vol); }
};
struct VolumePtr : std::unique_ptr<rslf_volume, VolumeDeleter> {
    using std::unique_ptr<rslf_volume, VolumeDeleter>::unique_ptr;
};
// The element type of a C-ABI entry's RSLF_ELEM_* argument, or the refusal of any other value.
inline int elem_of(int elem, Elem* out)
{
    switch (elem) {
    case RSLF_ELEM_F32:
        *out = Elem::F32;
        return RSLF_OK;
    case RSLF_ELEM_U8:
        *out = Elem::U8;
        return RSLF_OK;
    case RSLF_ELEM_U16:
        *out = Elem::U16;
        return RSLF_OK;
    }
    return fail(RSLF_ERR_INVALID_ARG, "element type %d: RSLF_ELEM_F32, _U8 or _U16", elem);
}
// What every pyramid entry shares: the host light field and the arguments of FineToCoarse's constructor and run()
// (rslf_fine_to_coarse.hpp:103-299).
struct F2cRequest {
    Elem elem = Elem::F32;
    const void* const* h_epis = nullptr;
    int V = 0, S = 0, U = 0, C = 0;
    size_t row_stride_bytes = 0;
    float d_min = 0.0f, d_max = 0.0f;
    int dim_d = 0;
    float epi_scale_factor = 1.0f;
    const rslf_params* p = nullptr;
    int max_pyr_depth = 0;
    int accept_all_last_scale = 0;
};
// What a pyramid is asked for beyond that; the defaults are "off": the reference's pyramid.  A kept run (rslf_f2c_run) holds
// the one copy of its options; the level loop and the sweep callables read the struct they are handed.
struct F2cOptions {
    int line_mode = RSLF_LINE_CONF_OFF;             // every level's sweep mode, and through plan::f2c_validity the plane its validity is read from
    int validity_rule = RSLF_F2C_VALID_COMPAT;      // RSLF_F2C_VALID_*; anything but COMPAT needs a kept run
    int subgrid = 0;                                // 1: every level's sweep in the sub-grid mode: the bound tightening, the validity and the fusion receive off-grid disparities
    bool keep_volumes = false;                      // a kept run keeps every level's normalised volume
    int peaks = 0;                                  // 1: a kept run's peak planes, of every level and of the fused map (rslf_f2c_run_host_pk) ...
    float uniqueness = 0.0f;                        // ... > 0: a level's valid pixels whose runner-up is within that ratio of the winner become
                                                    // invalid (k11_unique_mask) before the next level's bounds and the fusion read the plane
    float propagation_ratio = 0.0f;                 // > 0: every level's sweep gated by this ratio (rslf_f2c_run_host_pr; needs peaks)
    float cs_tol = 0.0f;                            // validity by cross-view consistency (rslf_f2c_run_host_cs): with cs_min_agree > 0, after a
    int cs_radius = 0, cs_min_agree = 0;            // level's rule and uniqueness, a valid pixel the other views contradict becomes invalid
    float derivative_weight = 0.0f;                 // > 0: a one-channel field goes down the pyramid as (x, |dx/du|, |dx/dv|) by this weight (K17,
                                                    // rslf_*_run_host_dv): three channels from the finest level's upload on
    int level_dilation = 1;                         // > 1: every level's SWEEP runs on the level's volume dilated along u by this factor (K16) and
    int dilation_kind = RSLF_DILATE_CUBIC;          // its planes come back to the level's own grid (K18; rslf_*_run_host_dl); the level chain is untouched
    int equalize_mode = 0;                          // RSLF_EQUALIZE_GAIN / _AFFINE: the finest level's upload is equalised per view, in place, before
    int equalize_ref_view = 0, equalize_joint = 0;  // anything else reads it (K19; rslf_*_run_host_eq): the view whose statistics are the target (-1: the
    float equalize_max_gain = 4.0f;                 // views' mean), one pair for the three channels, the clamp of the gain
};
// The host outputs of a pyramid, each nullable: the fused planes, the depth, every level's planes.
struct F2cHostOut {
    float* map_svu = nullptr;
    uint8_t* valid_svu = nullptr;
    int* n_levels = nullptr;
    const rslf_f2c_levels_out* levels = nullptr;
};
// One level of FineToCoarse as its sweep sees it, every pointer on the context's device.
struct F2cLevel {
    int V = 0, U = 0;
    rslf_params params;                 // slope_factor set (f2c.hpp:139)
    float scale = 1.0f;                 // the level's epi_scale_factor (dc.hpp:671-705)
    int C = 0;                          // channels of the level: the request's, or 3 with the derivative channels
    const float* raw_vsuc = nullptr;    // [V][S][U][C] raw values of the level
    const float* dmin_svu = nullptr;    // [S][V][U] ranges tightened from the level above; NULL on level 0
    const float* dmax_svu = nullptr;
    float* Ce_svu = nullptr;            // [S][V][U] results the sweep fills: edge confidence, disparities
    float* depth_svu = nullptr;
    const F2cOptions* options = nullptr;   // the run's: the sweep's modes; a sweep callable that cannot serve one refuses it by this
    float* Cl_svu = nullptr;            // the zero-filled [S][V][U] C_l plane of the level's sweep (NULL when the line mode is off)
    float* Cd_svu = nullptr;            // a kept run's [S][V][U] disparity confidence; NULL: the sweep has a plane of its own
    VolumePtr* vol_out = nullptr;         // a kept run with volumes: the sweep leaves the volume it ran on here
    const rslf_peaks* peaks = nullptr;    // a kept run with peak planes: the level's four [S][V][U] planes, for the sweep's peaks
                                          // mode (rslf_sweep_peaks; depth2d_run fills them with -1 / 0 first); NULL: mode off
    unsigned long long* withheld = nullptr;   // where the sweep leaves its count of withheld sources (gated levels only)
};
// What the level loop allocates per level and for the fusion.  The loop's own instance frees a level's confidences when the
// level is done and the rest on return, as it always did; a caller's instance (a kept run, rslf_f2c_run) keeps everything.
struct F2cKeptLevel {
    int V = 0, U = 0;
    float scale = 1.0f;                 // the level's epi_scale_factor as used
    float slope = 1.0f;                 // the slope factor the level's sweep ran with (f2c.hpp:139; rslf_f2c_run_consistency)
    DevBuf depth, valid, Ce, Cl;        // [S][V][U]: disparities, validity bytes, edge and line confidence (C_l empty when off)
    DevBuf Cd;                          // the disparity confidence (kept runs only)
    VolumePtr vol;                      // the normalised volume the sweep ran on (kept runs with volumes only)
    DevBuf pk_idx, pk_score, pk_runner_idx, pk_runner_score;   // the sweep's peak planes (kept runs with peaks only)
    unsigned long long withheld = 0;    // sources the level's sweep withheld (kept runs with a propagation ratio only)
    DevBuf cs_agree, cs_seen;           // the consistency gate's own counts at gate time, int32 (gated levels only)
    unsigned long long inconsistent = 0;   // pixels the gate made invalid (gated levels only)
};
struct F2cKept {
    std::vector<F2cKeptLevel> levels;   // finest first
    DevBuf fused_map, fused_valid;      // [S][V_0][U_0]
    DevBuf fused_pk_idx, fused_pk_score, fused_pk_runner_idx, fused_pk_runner_score, fused_level;   // [S][V_0][U_0] (k11_fuse_peaks; runs with peaks only)
    std::vector<float> view_gains;      // [S][C][2]: the (a, b) the equalisation applied to the finest level's upload (K19; empty when off)
};
// FineToCoarse constructor + run() + get_results() (rslf_fine_to_coarse.hpp:103-324) from the request's host EPIs into host
// planes: the pyramid, the bound tightening and the fusion on ctx, every level swept by `sweep`, which reports the level's
// stats.  keep (nullable): the owner of a kept run -- nothing is freed, every level also keeps C_d (and its volume,
// options.keep_volumes), the validity follows options.validity_rule (without keep it is COMPAT) and the host planes may be
// NULL.  With every option off, the loop queues what it always did.
int fine_to_coarse(rslf_ctx* ctx, const F2cRequest& req, const F2cOptions& options, const F2cHostOut& out, rslf_stats* stats,
                   F2cKept* keep, const std::function<int(const F2cLevel& level, rslf_stats* level_stats)>& sweep);
// What every pyramid entry refuses of the level dilation before a device is touched: the factor, the kind, a line mode with it.
int check_level_dilation(const F2cOptions& options);
// The loop on one context: each level a volume of its own, packed from the raw level and swept by depth2d_run.
int fine_to_coarse_one_context(rslf_ctx* ctx, const F2cRequest& req, const F2cOptions& options, const F2cHostOut& out,
                               rslf_stats* stats, F2cKept* keep);

// rslf_derivative.hip
// The raw form of the derivative channels (K17), enqueued on the context's stream: a dense level d_in [V][S][U] (integer
// elements: integer values held as floats) becomes d_out [V][S][U][3].  hi: the cap of float elements (derivative_hi_f32).
int derivative_channels_raw(rslf_ctx* ctx, const float* d_in, Elem e, int V, int S, int U, float weight, float hi, float* d_out);

// rslf_equalize.hip
// What every pyramid entry refuses of the equalisation before a device is touched: the mode, the reference view, the gain's
// clamp, joint with one channel, a field whose V * U the statistic cannot count exactly.  Mode 0 (off) refuses nothing.
int check_equalize(const F2cOptions& options, int V, int S, int U, int C);
// The dense form of the per-view equalisation (K19) in place, awaited: statistics, coefficients on the host, apply.  hi: the
// cap of float elements (> 0); an integer type's own otherwise.  h_a_b [S][C][2] receives the coefficients (nullable).
int equalize_views_raw(rslf_ctx* ctx, float* d_inout, Elem e, int V, int S, int U, int C, float hi, int mode, int ref_view, int joint,
                       float max_gain, float* h_a_b);

// rslf_multi.hip
void multi_free_dev(rslf_multi::Dev& d);
// a copy between two devices of a multi object (or within one), queued on `st`: a plain device copy on one device, else a
// peer copy (direct over xGMI where rslf_multi_create enabled peer access, staged through the host by the runtime where not)
hipError_t multi_copy(rslf_multi* m, void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st);

}  // namespace rslf

// A finished fine-to-coarse run held on one device (rslf_f2c_keep.hip).  Bound to the device, not to a context.
struct rslf_f2c_run {
    int device = 0;
    int S = 0, C = 0, elem = RSLF_ELEM_F32;
    rslf::F2cOptions options;   // what the run was made with: the loop read them, the getters do
    rslf_params params;   // as given: the getters' cut_shadows / shadow_level
    rslf::F2cKept kept;
};
