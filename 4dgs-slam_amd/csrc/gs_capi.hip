// gs_capi.hip -- host orchestration + the extern "C" boundary declared in include/gs_rasterizer.h.
// Mirrors CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (DGR/cuda_rasterizer/rasterizer_impl.cu:141-153,198-344,348-455) with an MI355X-first pipeline:
//
//   forward : F1 preprocess (+ per-block tile histogram rows, + block sums) -> F1b column scan -> F2 single-pass scans (+ host mailbox)
//             -> F3 scatter -> [F4 sort of lists > 1024] -> F5 tile kernel (sorts its own list, composites, checkpoints),
//             all enqueued speculatively on a binning buffer sized from the previous frame; the host then reads R from the
//             mailbox and only redoes F3..F5 if the scan kernel flagged the capacity as too small
//   backward: B1 gradient pass, one block per 128-entry chunk of a tile list (swap/DPP reductions, per-instance slots)
//             -> B2 per-Gaussian gather + geometry -> pose-gradient sum
//   extras  : raw-parameter entry points (fused prologue), fused L1 losses, fused Adam, exact 3-NN (simple_knn)
//
// No global 64-bit radix sort, no float atomics, no cooperative-groups block trees.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <sched.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>

#include "../../include/gs_rasterizer.h"
#include "../../include/simple_knn.h"
#include "gs_backward.h"
#include "gs_views.h"
#include "gs_knn.h"
#include "gs_loss.h"
#include "gs_hexplane.h"
#include "gs_hexplane_binned.h"
#include "gs_linear.h"
#include "gs_mlp.h"
#include "gs_dense.h"
#include "../../include/dense_layers.h"
#include "gs_nodes.h"
#include "../../include/slam_losses.h"
#include "../../include/slam_map.h"
#include "gs_map.h"
#include "../../include/frame_io.h"
#include "gs_frame.h"
#include "../../include/video_io.h"
#include "gs_jpeg.h"
#include "gs_jpeg_decode.h"
#include "gs_png.h"
#include "../../include/stereo_depth.h"
#include "gs_stereo.h"
#include "../../include/multiview_depth.h"
#include "gs_sweep.h"
#include "../../include/optical_flow.h"
#include "gs_raft.h"
#include "gs_gma.h"
#include "../../include/segmentation.h"
#include "gs_yolo.h"
#include "../../include/perceptual.h"
#include "gs_lpips.h"
#include "../../include/motion_segmentation.h"
#include "gs_motion.h"
#include "../../include/visual_odometry.h"
#include "gs_odometry.h"
#include "../../include/relocalisation.h"
#include "gs_reloc.h"
#include "../../include/loop_closure.h"
#include "gs_loop.h"
#include "../../include/feature_matching.h"
#include "gs_features.h"

namespace gsr {

static thread_local std::string g_last_error;

#define GSR_HIP_CHECK(expr)                                                                              \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
            return GSR_ERR_HIP;                                                                          \
        }                                                                                                \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: `done` holds one bit per device ordinal, so a process
// that drives several GPUs sets it on each of them (a process-wide flag left the second device at the 64 KB default and the 156 KB launch
// failed there); atomic: the entry points may be called from several host threads.
static int ensure_dynamic_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& done)
{
    int dev = 0;
    GSR_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        GSR_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done.fetch_or(bit, std::memory_order_release);
    }
    return 0;
}

static size_t binning_bytes(size_t carve_R, size_t cap_sorted, size_t ntiles)
{
    return (size_t)(carve_binning(nullptr, carve_R, cap_sorted, ntiles).end - (char*)nullptr) + 256;
}
template <typename F>
static size_t required(F&& f)
{
    char* p = nullptr;
    f(p);
    return reinterpret_cast<size_t>(p) + 256;
}

// ---- workspaces that only the host carves ------------------------------------------------------------------------------------------
// One layout function per workspace: it takes the shape arguments and a base and returns typed pointers plus the total bytes. The
// *_workspace_size entry point runs it on a null base (null pointers, the same offsets), the launching entry point on the caller's pointer;
// no offset, rounding or slack of such a workspace is written anywhere else. Regions lie in the order they are taken, each starting on a
// multiple of `unit` bytes from the base. align_base: the entry point accepts any base, the carver rounds it up to `unit` and the size pays
// one unit for that. Where a layout function returns its struct as a braced list of take() calls, the members' order is the regions' order
// (a braced list is evaluated left to right). (GeomState / ImageState / carve_binning above are not of this kind: the multi-view kernels
// carve them on the device.)
struct Carver {
    char* base;
    size_t unit, slack, off = 0;
    Carver(const void* workspace, size_t unit_, bool align_base = false) : unit(unit_), slack(align_base ? unit_ : 0)
    {
        const size_t a = reinterpret_cast<size_t>(workspace);
        base = reinterpret_cast<char*>(align_base ? up(a) : a);
    }
    size_t up(size_t v) const { return (v + unit - 1) & ~(unit - 1); }
    template <typename T> T* take(size_t count)
    {
        off = up(off);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    char* nested(size_t bytes) { return take<char>(bytes); }                      // a sub-workspace: another layout function carves it
    size_t bytes() const { return std::max(off + slack, unit); }                  // the last region ends with its data; never 0
    size_t bytes_padded() const { return std::max(up(off) + slack, unit); }       // the last region rounded up as well
};
// What the entry points that receive the byte count of their workspace ask of it (tests match on the text)
static bool workspace_fits(const char* who, const char* size_fn, const void* workspace, size_t workspace_bytes, size_t need)
{
    if (workspace_bytes >= need && !(reinterpret_cast<size_t>(workspace) & 15)) return true;
    g_last_error = std::string(who) + ": workspace must be 16-byte aligned and hold " + std::to_string(need) + " bytes (" + size_fn + "), got " +
                   std::to_string(workspace_bytes);
    return false;
}

// ---- per-kernel timing with events on the launch stream ---------------------------------------------------------
enum KernelId { K_PREPROCESS = 0, K_SCAN, K_SCATTER, K_SORT, K_RENDER_FWD, K_RENDER_BWD, K_GEOM_BWD, K_KNN, K_FRAME_PREPARE,
                K_SWEEP_CENSUS, K_SWEEP_COST, K_SWEEP_PATHS, K_SWEEP_SELECT, K_ODO_PYRAMID, K_ODO_SUMS, K_ODO_SOLVE, K_JPEGD_ENTROPY, K_JPEGD_PIXELS,
                K_COUNT };
static const char* const kKernelNames[K_COUNT] = {"preprocess_fwd", "scan", "scatter_instances", "sort_tiles",
                                                  "render_fwd", "render_bwd", "geometry_bwd", "knn_total", "frame_prepare",
                                                  "sweep_census", "sweep_cost", "sweep_paths", "sweep_select",
                                                  "odometry_pyramid", "odometry_sums", "odometry_solve",
                                                  "jpeg_decode_entropy", "jpeg_decode_pixels"};
struct Profiler {
    unsigned mask = 0;   // bit i set => kernel id i is timed
    struct Rec { hipEvent_t a, b; int id; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[K_COUNT] = {0};
    int calls[K_COUNT] = {0};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
    void drain()
    {
        for (auto& r : pending) {
            (void)hipEventSynchronize(r.b);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { total_ms[r.id] += ms; calls[r.id]++; }
            pool.push_back(r.a); pool.push_back(r.b);
        }
        pending.clear();
    }
};
static Profiler g_prof;
struct ScopedKernelTimer {
    int id; hipStream_t s; hipEvent_t a{}, b{}; bool on;
    ScopedKernelTimer(int id_, hipStream_t s_) : id(id_), s(s_), on((g_prof.mask >> id_) & 1u)
    {
        if (on) { a = g_prof.get(); b = g_prof.get(); (void)hipEventRecord(a, s); }
    }
    ~ScopedKernelTimer()
    {
        if (on) { (void)hipEventRecord(b, s); g_prof.pending.push_back({a, b, id}); if (g_prof.pending.size() > 4096) g_prof.drain(); }
    }
};

static int debug_sync(int debug, hipStream_t s, const char* what)
{
    // CHECK_CUDA(..., debug) of the reference (auxiliary.h:166-173): synchronise after every stage when debugging.
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && debug) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { g_last_error = std::string(what) + ": " + hipGetErrorString(e); return GSR_ERR_HIP; }
    return 0;
}
#define GSR_STAGE(what) do { int _r = debug_sync(debug, stream, what); if (_r) return _r; } while (0)

// Host mailbox: 8 words of pinned, host-coherent memory per host thread; word 4 carries the sequence number of the
// forward call whose header (words 0-3) is valid. Plus the allocation size that was enough last time (speculative
// binning allocation while the GPU is still busy with the preprocess).
// ... all of it per (host thread, device): a thread that renders on several GPUs gets one mailbox and one capacity estimate per device
// (the mailbox's device pointer is the one hipHostGetDevicePointer returns for THAT device).
// ... and per view SLOT of the multi-view entry point (slot 0 = the single-view calls): the v-th view of consecutive mapping iterations
// looks alike, the views of one iteration do not.
struct SpecState { uint32_t* mailbox = nullptr; uint32_t* mailbox_dev = nullptr; uint32_t seq = 0; size_t last_R_alloc = 0; uint32_t last_max_tile = 0; };
constexpr int VIEW_SLOT_GROUPS = 4;                             // gsr_set_option("view_slot_group", g): a caller that splits one iteration's views over several calls names the call
constexpr int SPEC_SLOTS = 1 + 2 * MAX_VIEWS * VIEW_SLOT_GROUPS;
static thread_local SpecState t_spec[16][SPEC_SLOTS];   // [device][0 = single-view calls | per group: 1..V views of a batch | MAX_VIEWS+1.. views of a flow batch]
static thread_local int t_view_slot_group = 0;
static int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    return dev;
}
// the capacity estimate and mailbox of view slot `slot` of this thread on the current device
static SpecState& spec_state(int slot) { return t_spec[current_device()][slot]; }
static thread_local bool t_use_mailbox = true;
static thread_local bool t_speculate = true;
// Lazy mode (gsr_set_option("lazy", 1)): a speculative forward pass returns WITHOUT waiting for the scan kernel's header -- no host
// synchronisation at all, which is also what makes the call capturable in a hipGraph. The value returned in place of num_rendered is
// then the capacity the binning buffer was laid out for (an upper bound of R; gsr_backward only sizes its grid from it, the kernels
// read the true counts from the device header). If a frame outgrows the capacity, the speculative kernels and both backward kernels
// of that frame exit at once (outputs / gradients of THAT call are undefined) and the sticky overflow counter in the mailbox is
// bumped: a caller that uses lazy mode polls gsr_forward_status() at a convenient point and repeats the affected work eagerly.
static thread_local bool t_lazy = false;
static thread_local int t_cap_margin_permille = 125;   // head room of a speculative binning buffer over the last frame's count (gsr_set_option)
static thread_local int t_cap_tile_margin_permille = -1;  // head room of the longest tile list (which picks the sort kernels); < 0: max(250, cap_margin_permille)
static inline unsigned tile_margin() { return (unsigned)(t_cap_tile_margin_permille >= 0 ? t_cap_tile_margin_permille : std::max(250, t_cap_margin_permille)); }
static thread_local int t_cap_test_shrink_permille = 0; // TEST facility: > 0 lays speculative buffers out for that fraction of the last count (forces overflows)
static thread_local int t_cap_floor = 0;               // smallest speculative capacity, in instances (gsr_set_option "cap_floor")
static inline size_t spec_capacity(size_t last)
{
    if (t_cap_test_shrink_permille > 0) return (size_t)((unsigned long long)last * (unsigned)t_cap_test_shrink_permille / 1000ull) + 1;
    return std::max(last + (size_t)((unsigned long long)last * (unsigned)t_cap_margin_permille / 1000ull) + 4096, (size_t)t_cap_floor);
}
static thread_local bool t_options_read = false;
static thread_local unsigned t_views_batched = 0;
// Process-wide options (gsr_set_option may change them from any thread):
// render_bwd's work items: full pieces in tile order, then the partial pieces longest first at the end of every XCD's sequence (gs_device.h:
// item_block_*; one extra block of the scatter launch ranks them). GSR_ORDER_ITEMS=0: tile order, as rounds 2-5 (A/B runs; the results are
// bit-identical either way)
static std::atomic<bool> g_order_items{getenv("GSR_ORDER_ITEMS") ? getenv("GSR_ORDER_ITEMS")[0] != '0' : true};
// SH coefficient rows move through LDS in preprocess_fwd / geometry_bwd (gs_backward.h); GSR_SH_ROWS=0: per lane (bit-identical results)
static std::atomic<bool> g_sh_rows{getenv("GSR_SH_ROWS") ? getenv("GSR_SH_ROWS")[0] != '0' : true};
// HexPlane plane gradients as fixed-point integer sums (gs_hexplane_binned.h: HexOrd): bitwise the same run to run. 0: float atomics (rounds 1-5)
static std::atomic<int> g_hex_ordered{getenv("GSR_HEX_ORDERED") ? (getenv("GSR_HEX_ORDERED")[0] != '0' ? 1 : 0) : 1};
static void read_option_env()
{
    if (t_options_read) return;
    t_options_read = true;
    if (const char* e = getenv("GSR_MAILBOX")) t_use_mailbox = e[0] != '0';
    if (const char* e = getenv("GSR_SPECULATE")) t_speculate = e[0] != '0';
    if (const char* e = getenv("GSR_LAZY")) t_lazy = e[0] != '0';
}
// The options of one rasterizer call, read once at its entry point: every launch of the call sees the same values.
struct Options { bool speculate, lazy, mailbox, order_items, sh_rows; };
static Options read_options()
{
    read_option_env();
    return {t_speculate, t_lazy, t_use_mailbox, g_order_items.load(std::memory_order_relaxed), g_sh_rows.load(std::memory_order_relaxed)};
}

// gsr_track_step (include/slam_map.h): what replaces tau_sum_kernel at the end of the backward pass
struct TrackTail { const float* exposure_partials; float* dL_dexposure; CameraStepArgs step; };
// The per-call state of the rasterizer orchestration, built at the extern "C" entry point and handed down.
struct Call {
    Options opt;
    SpecState* spec = nullptr;                    // capacity estimate + mailbox of the (device, view slot) a forward pass renders for
    const int* flow_clip = nullptr;               // a flow view's tile rectangle (gsr_view.flow_clip); NULL = the whole image
    const TrackLossArgs* track_loss = nullptr;    // gsr_track_step: the loss epilogue of render_fwd (render_fwd_track_kernel)
    const TrackTail* track_tail = nullptr;        // gsr_track_step: track_tail_kernel in place of tau_sum_kernel
};

// small launches are latency-bound: the per-Gaussian kernels then request every row they may need up front (gs_forward.h)
constexpr int EAGER_MAX_P = 512 * 1024;
constexpr int DEAL_HEAVY = 1;
// where tile lists of up to `longest_list` entries get sorted (gs_views.h: SortTier)
static SortTier sort_tier(uint32_t longest_list)
{
    if (longest_list <= (uint32_t)SORT_SMALL_CAP) return {SortTier::NONE, 0};
    if (longest_list <= (uint32_t)SORT_MID_CAP) return {SortTier::MID, 0};
    return {SortTier::FULL, longest_list > (uint32_t)SORT_LDS_CAP ? (longest_list + (uint32_t)SORT_LDS_CAP - 1) / (uint32_t)SORT_LDS_CAP : 0};
}
// Longest tile list the speculative launches are sized for, from the last frame's (plus head room): the longest of its tier (and chunk grid)
static uint32_t tile_list_capacity(uint32_t last_max_tile)
{
    const SortTier t = sort_tier(last_max_tile + (uint32_t)((unsigned long long)last_max_tile * tile_margin() / 1000ull));
    return t.kind == SortTier::NONE ? (uint32_t)SORT_SMALL_CAP : t.kind == SortTier::MID ? (uint32_t)SORT_MID_CAP : std::max(t.chunks, 1u) * (uint32_t)SORT_LDS_CAP;
}
// preprocess_fwd's dynamic LDS at its largest: the tile histogram of a frame of HIST_LDS_TILES tiles, then one SH window per wave
constexpr size_t PRE_LDS_MAX = (((size_t)HIST_LDS_TILES * sizeof(uint32_t) + 15) & ~size_t(15)) + (size_t)(GB / 64) * SH_WIN_FLOATS * sizeof(float);
static_assert(PRE_LDS_MAX <= 160 * 1024, "preprocess_fwd's LDS must fit gfx950's 160 KiB per workgroup");

static FwdPlan plan_forward(const Options& opt, int P, int D, int M, int width, int height, bool flow, bool colors_precomp)
{
    FwdPlan p;
    p.d = view_dims(P, width, height); p.eager = P <= EAGER_MAX_P ? 1 : 0; p.wide_offsets = p.d.nblocks > TO_SEGS * 16;
    p.lds_hist = use_lds_hist((size_t)p.d.T); p.hist_lds_bytes = p.lds_hist ? (size_t)p.d.T * sizeof(uint32_t) : 0;
    p.order_items = opt.order_items && p.lds_hist;
    const bool fwd_tiles = p.order_items && p.d.T / 8 >= ORDER_FWD_MIN_BAND;
    p.order_fwd = fwd_tiles ? 1 + DEAL_HEAVY : 0; p.order_word = p.order_items ? 1 | (fwd_tiles ? 2 | DEAL_HEAVY << 2 : 0) : 0;
    p.sh_win = opt.sh_rows && p.lds_hist && D > 0 && !colors_precomp && (M == 9 || M == 16) && !flow;
    p.sh_win_offset = p.sh_win ? (int)((p.hist_lds_bytes + 15) & ~size_t(15)) : 0;
    p.pre_lds = p.sh_win ? (size_t)p.sh_win_offset + (size_t)(GB / 64) * SH_WIN_FLOATS * sizeof(float) : p.hist_lds_bytes;
    return p;
}
// f(shape): the <SEGS, RMAX> of the plan's tile_offsets kernel, as a type (gs_views.h: OffsetsShape)
template <typename F> static void with_tile_offsets(const FwdPlan& p, F&& f) { if (p.wide_offsets) f(OffsetsShape<TO_SEGS_BIG, 32>{}); else f(OffsetsShape<TO_SEGS, 16>{}); }
// f(k): the <RAW, PRE> of the call's preprocess / geometry kernel, as a type (gs_views.h: RawPre) -- <true, true> for raw inputs in delta_mode, <true, false>
// for other raw inputs, <false, false> for activated ones, which RAW_ONLY leaves out (the batched kernels exist for raw inputs only)
template <bool RAW_ONLY = false, typename F> static auto with_raw_pre(bool raw, bool delta_mode, F&& f)
{
    if (raw && delta_mode) return f(RawPre<true, true>{});
    if constexpr (RAW_ONLY) return f(RawPre<true, false>{});
    else return raw ? f(RawPre<true, false>{}) : f(RawPre<false, false>{});
}
// A preprocess launch with the plan's dynamic LDS. The SH windows take it beyond the 64 KB default: the attribute is a cap set once per (kernel,
// device), to the largest frame's bytes, so that a later frame with more tiles than the first still launches (a launch passes only what it uses)
template <auto KERNEL, typename... Args> static int launch_preprocess(const FwdPlan& p, dim3 grid, hipStream_t stream, const Args&... args)
{
    static std::atomic<unsigned long long> raised;   // (one per kernel instantiation)
    if (p.sh_win) { const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), (int)PRE_LDS_MAX, raised); if (rc) return rc; }
    hipLaunchKernelGGL(KERNEL, grid, dim3(GB), p.pre_lds, stream, args...);
    return 0;
}
// The fields of the preprocess / geometry kernels' arguments that do not depend on the view, the rest zero: a single-view call then sets the buffer
// pointers on the host, a batch leaves them to the device (gs_views.h: view_geom / view_image)
static PreprocessArgs preprocess_args(const FwdPlan& p, int D, int M, float scale_modifier, float tan_fovx, float tan_fovy, int prefiltered, const RawInputs& raw)
{
    PreprocessArgs a{};
    a.P = p.d.P; a.D = D; a.M = M; a.W = p.d.W; a.H = p.d.H; a.gx = p.d.gx; a.gy = p.d.gy;
    a.scale_modifier = scale_modifier; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
    a.focal_y = p.d.H / (2.0f * tan_fovy); a.focal_x = p.d.W / (2.0f * tan_fovx);   // rasterizer_impl.cu:225-226
    a.prefiltered = prefiltered; a.eager = p.eager; a.sh_win_offset = p.sh_win_offset; a.raw = raw;
    return a;
}
static GeomBwdArgs geom_bwd_args(const Options& opt, const ViewDims& d, int D, int M, float scale_modifier, float tan_fovx, float tan_fovy, bool pose_only, const RawInputs& raw, int scale_dim)
{
    GeomBwdArgs a{};
    a.P = d.P; a.D = D; a.M = M; a.W = d.W; a.H = d.H; a.scale_modifier = scale_modifier;
    a.focal_y = d.H / (2.0f * tan_fovy); a.focal_x = d.W / (2.0f * tan_fovx); a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
    a.pose_only = pose_only ? 1 : 0; a.sh_rows = opt.sh_rows ? 1 : 0; a.raw = raw; a.rawg.scale_dim = scale_dim;
    return a;
}

static int ensure_mailbox(SpecState& s)
{
    if (!s.mailbox) {
        GSR_HIP_CHECK(hipHostMalloc((void**)&s.mailbox, 8 * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable));
        memset(s.mailbox, 0, 8 * sizeof(uint32_t));
        GSR_HIP_CHECK(hipHostGetDevicePointer((void**)&s.mailbox_dev, s.mailbox, 0));
    }
    return 0;
}

// the header of the forward pass numbered `seq` of slot `s`; use_mailbox: the call's option, cleared (for this call and the thread) when
// the mailbox turns out not to work
static int wait_for_header(hipStream_t stream, const SpecState& s, bool& use_mailbox, const uint32_t* device_header, uint32_t seq, uint32_t out[4])
{
    if (use_mailbox) {
        // spin on the mailbox (the scan kernel is a few microseconds away when the GPU is not backed up); after ~1e5 polls the wait is
        // evidently long, so the core is yielded between polls; the stream is checked now and then so that a faulted / finished stream
        // cannot hang us
        for (unsigned long long spins = 0;; spins++) {
            if (__atomic_load_n(&s.mailbox[4], __ATOMIC_ACQUIRE) == seq) {
                for (int i = 0; i < 4; i++) out[i] = __atomic_load_n(&s.mailbox[i], __ATOMIC_RELAXED);
                return 0;
            }
            if (spins > 100000ull) sched_yield();
            if ((spins & 0xFFFFF) == 0xFFFFF) {
                hipError_t q = hipStreamQuery(stream);
                if (q == hipSuccess) {   // stream drained: the store must be visible by now, otherwise fall back for good
                    if (__atomic_load_n(&s.mailbox[4], __ATOMIC_ACQUIRE) == seq) continue;
                    t_use_mailbox = use_mailbox = false;
                    break;
                }
                if (q != hipErrorNotReady) { g_last_error = std::string("stream error while waiting for the header: ") + hipGetErrorString(q); return GSR_ERR_HIP; }
            }
        }
    }
    GSR_HIP_CHECK(hipMemcpyAsync(out, device_header, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GSR_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

// The header the host waited for: the frame's counts, which become the slot's estimates for the next frame
struct FrameCounts { uint32_t R, R_alloc, flags, max_tile; };
static int absorb_header(SpecState& spec, const uint32_t hdr[4], const char* who, FrameCounts& f)
{
    f = {hdr[HDR_R], hdr[HDR_R_ALLOC], hdr[HDR_FLAGS], hdr[HDR_MAX_TILE]};
    if (f.R > 0x7fffffffu || f.R_alloc > 0x7fffffffu) { g_last_error = std::string(who) + ": more than 2^31 instances"; return GSR_ERR_INVALID_ARGUMENT; }
    spec.last_R_alloc = std::max<size_t>(1, f.R_alloc > f.R ? f.R_alloc : f.R);     // (never 0: 0 means "no estimate yet"; a frame may legitimately have no instance)
    spec.last_max_tile = f.max_tile;
    return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

const char* gsr_last_error(void) { return g_last_error.c_str(); }
const char* gsr_version(void) { return "gs_rasterizer_hip 0.1 (gfx950)"; }

size_t gsr_geometry_buffer_size(int P) { return required([&](char*& p) { GeomState::from(p, (size_t)P); }); }
size_t gsr_image_buffer_size(int width, int height, int P)
{
    const size_t T = (size_t)((width + TILE_X - 1) / TILE_X) * ((height + TILE_Y - 1) / TILE_Y);
    return required([&](char*& p) { ImageState::from(p, (size_t)width * height, T, (size_t)P); });
}
size_t gsr_binning_buffer_size(int R_alloc) { return binning_bytes((size_t)R_alloc, (size_t)R_alloc, (size_t)65536); }   // sized for frames of up to 65 536 tiles (4096 x 4096 pixels)

int gsr_set_option(const char* name, int value)
{
    read_option_env();
    if (!name) { g_last_error = "gsr_set_option: null name"; return GSR_ERR_INVALID_ARGUMENT; }
    const std::string n(name);
    if (n == "views_batched") return (int)t_views_batched;     // read-only: multi-view calls of this thread that took the one-launch-per-stage path
    if (n == "hex_ordered") {                                  // process-wide (the workspace sizes depend on it); value < 0 only reads
        const int old_ordered = g_hex_ordered.load();
        if (value >= 0) g_hex_ordered.store(value ? 1 : 0);
        return old_ordered;
    }
    if (n == "cap_margin_permille") {
        const int old_margin = t_cap_margin_permille;
        if (value >= 0) t_cap_margin_permille = value > 4000 ? 4000 : value;
        return old_margin;
    }
    if (n == "cap_tile_margin_permille") {
        const int old_margin = t_cap_tile_margin_permille < 0 ? 1000000 : t_cap_tile_margin_permille;      // 1000000 = "follow cap_margin_permille"
        if (value >= 1000000) t_cap_tile_margin_permille = -1;
        else if (value >= 0) t_cap_tile_margin_permille = value > 16000 ? 16000 : value;
        return old_margin;
    }
    if (n == "view_slot_group") {
        const int old_group = t_view_slot_group;
        if (value >= 0) t_view_slot_group = value >= VIEW_SLOT_GROUPS ? VIEW_SLOT_GROUPS - 1 : value;
        return old_group;
    }
    if (n == "cap_floor") {
        const int old_floor = t_cap_floor;
        if (value >= 0) t_cap_floor = value > (1 << 26) ? (1 << 26) : value;
        return old_floor;
    }
    if (n == "cap_test_shrink_permille") {
        const int old_shrink = t_cap_test_shrink_permille;
        if (value >= 0) t_cap_test_shrink_permille = value > 1000 ? 1000 : value;
        return old_shrink;
    }
    if (n == "order_items" || n == "sh_rows") {               // process-wide
        std::atomic<bool>& opt = n == "order_items" ? g_order_items : g_sh_rows;
        const int old = opt.load(std::memory_order_relaxed) ? 1 : 0;
        if (value >= 0) opt.store(value != 0, std::memory_order_relaxed);
        return old;
    }
    bool* opt = n == "speculate" ? &t_speculate : n == "lazy" ? &t_lazy : n == "mailbox" ? &t_use_mailbox : nullptr;
    if (!opt) { g_last_error = "gsr_set_option: unknown option '" + n + "' (speculate, lazy, mailbox, order_items, sh_rows, cap_margin_permille, cap_tile_margin_permille, cap_floor, view_slot_group)"; return GSR_ERR_INVALID_ARGUMENT; }
    const int old = *opt ? 1 : 0;
    if (value >= 0) *opt = value != 0;
    return old;
}

int gsr_forward_status(unsigned int* overflow_count, unsigned int* last_num_rendered)
{
    const uint32_t* mb = spec_state(0).mailbox;
    if (overflow_count) *overflow_count = mb ? __atomic_load_n(&mb[5], __ATOMIC_ACQUIRE) : 0u;
    if (last_num_rendered) *last_num_rendered = mb ? __atomic_load_n(&mb[0], __ATOMIC_ACQUIRE) : 0u;
    return 0;
}

int gsr_forward_status_views(unsigned int* overflow_count_total)
{
    const int dev = current_device();
    unsigned int total = 0;
    for (int slot = 0; slot < SPEC_SLOTS; slot++)
        if (const uint32_t* mb = t_spec[dev][slot].mailbox) total += __atomic_load_n(&mb[5], __ATOMIC_ACQUIRE);
    if (overflow_count_total) *overflow_count_total = total;
    return 0;
}

/* Dev: per view slot of this thread and device, 8 words: mailbox R, flags, R_alloc, max tile, seq, overflow count | the host's estimates
 * last_R_alloc, last_max_tile. out: [slots][8]; returns the number of slots. */
int gsr_debug_view_slots(unsigned int* out, int max_slots)
{
    const int dev = current_device();
    const int n = max_slots < SPEC_SLOTS ? max_slots : SPEC_SLOTS;
    for (int slot = 0; slot < n; slot++) {
        const SpecState& s = t_spec[dev][slot];
        for (int k = 0; k < 6; k++) out[slot * 8 + k] = s.mailbox ? __atomic_load_n(&s.mailbox[k], __ATOMIC_ACQUIRE) : 0u;
        out[slot * 8 + 6] = (unsigned int)s.last_R_alloc; out[slot * 8 + 7] = s.last_max_tile;
    }
    return n;
}

int gsr_profile_enable(int kernel_mask) { g_prof.mask = (unsigned)kernel_mask; return K_COUNT; }
void gsr_profile_reset(void)
{
    g_prof.drain();
    for (int i = 0; i < K_COUNT; i++) { g_prof.total_ms[i] = 0; g_prof.calls[i] = 0; }
}
int gsr_profile_read(const char** names, float* total_ms, int* calls, int cap)
{
    g_prof.drain();
    int n = 0;
    for (int i = 0; i < K_COUNT && n < cap; i++, n++) {
        if (names) names[n] = kKernelNames[i];
        if (total_ms) total_ms[n] = (float)g_prof.total_ms[i];
        if (calls) calls[n] = g_prof.calls[i];
    }
    return n;
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, unsigned char* present, void* stream_)
{
    (void)projmatrix;
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) { g_last_error = "gsr_mark_visible: null argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P == 0) return 0;
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, viewmatrix, present);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"

static RawInputs to_device_view(const gsr_raw_inputs* in, const int* flow_clip)
{
    RawInputs r{};
    if (in) {
        r.xyz = in->xyz; r.log_scales = in->log_scales; r.scale_dim = in->scale_dim; r.raw_rot = in->raw_rotations;
        r.logit_opacity = in->logit_opacity; r.f_dc = in->features_dc; r.f_rest = in->features_rest;
        r.dyn_slot = in->dyn_slot; r.dx = in->dx; r.ds = in->ds; r.dr = in->dr; r.gather = in->gather;
        r.flow_dx2 = in->flow_dx2; r.flow_proj1 = in->flow_proj1; r.flow_proj2 = in->flow_proj2;
        r.flow_clip = in->flow_proj1 ? flow_clip : nullptr;
        r.delta_mode = in->delta_mode; r.delta_stride = in->delta_stride;
    }
    return r;
}
static bool raw_inputs_ok(const gsr_raw_inputs* in, int M)
{
    const bool flow = in->flow_proj1 != nullptr;
    if (flow && (!in->flow_proj2 || M != 1 || (in->flow_dx2 && !in->dyn_slot) || in->delta_mode || in->delta_stride)) return false;
    if ((in->delta_mode != 0 && in->delta_mode != 1) || in->delta_stride < 0 || (in->delta_stride && (in->delta_stride < 4 || !in->delta_mode)) ||
        (in->delta_mode && in->gather)) return false;
    return in->xyz && in->log_scales && (in->scale_dim == 1 || in->scale_dim == 3) && in->raw_rotations && in->logit_opacity &&
           (flow || (in->features_dc && (M == 1 || in->features_rest))) && ((!in->dx && !in->ds && !in->dr) || in->dyn_slot || in->delta_mode);
}

// forward_impl's inputs: gsr_forward's arrays (raw == NULL), or gsr_forward_raw's descriptor (the arrays are then NULL)
struct FwdInputs {
    const float* means3D = nullptr; const float* shs = nullptr; const float* colors_precomp = nullptr; const float* opacities = nullptr;
    const float* scales = nullptr; const float* rotations = nullptr; const float* cov3D_precomp = nullptr; int prefiltered = 0;
    const gsr_raw_inputs* raw = nullptr;
};
struct FwdCamera { const float* viewmatrix; const float* projmatrix; const float* cam_pos; float tan_fovx, tan_fovy; const float* projmatrix_raw = nullptr; /* backward only */ };
struct FwdOutputs { float* color; float* depth; float* opacity; int* radii; int* n_touched; };
// backward_impl: what the forward pass left (radii NULL: the geometry buffer's own), the cotangents of its outputs, the gradients wanted. Intermediate ones the caller does not
// want stay NULL (dL_dconic, dL_dcolor, dL_ddepth, dL_dcov3D; dL_dtau when dL_dtau_sum is given): the kernel then keeps them in registers only. gsr_backward requires them all.
struct BwdState { char* geom_buffer; char* binning_buffer; char* image_buffer; const int* radii; int R; };
struct BwdCotangents { const float* dL_dpix; const float* dL_dpix_depth; };
struct BwdGrads {
    float *dL_dmean2D = nullptr, *dL_dconic = nullptr, *dL_dopacity = nullptr, *dL_dcolor = nullptr, *dL_ddepth = nullptr, *dL_dmean3D = nullptr, *dL_dcov3D = nullptr;
    float *dL_dsh = nullptr, *dL_dscale = nullptr, *dL_drot = nullptr, *dL_dtau = nullptr, *dL_dtau_sum = nullptr;
};
// view `w` of a multi-view call as a single-view descriptor: the call's raw inputs with the view's deltas and flow pointers
static gsr_raw_inputs view_raw_inputs(gsr_raw_inputs one, const gsr_view& w)
{
    one.dx = w.dx; one.ds = w.ds; one.dr = w.dr; one.flow_dx2 = w.flow_dx2; one.flow_proj1 = w.flow_proj1; one.flow_proj2 = w.flow_proj2;
    return one;
}
// ... and as a row of the batched kernels' table: what the forward and the backward pass both read
static void fill_view_slot(ViewSlot& s, const gsr_view& w)
{
    s.viewmatrix = w.viewmatrix; s.projmatrix = w.projmatrix; s.projmatrix_raw = w.projmatrix_raw; s.cam_pos = w.cam_pos;
    s.dx = w.dx; s.ds = w.ds; s.dr = w.dr;
    s.flow_dx2 = w.flow_dx2; s.flow_proj1 = w.flow_proj1; s.flow_proj2 = w.flow_proj2;
    s.geom = w.geom_buffer; s.image = w.image_buffer; s.binning = w.binning_buffer; s.radii = w.radii;
}
struct FwdAllocs { gsr_alloc_fn geometry; void* geometry_user; gsr_alloc_fn binning; void* binning_user; gsr_alloc_fn image; void* image_user; };

static int forward_impl(Call& c, const FwdAllocs& alloc, int P, int D, int M, const float* background, int width, int height, const FwdInputs& in,
                        float scale_modifier, const FwdCamera& cam, FwdOutputs out, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const gsr_raw_inputs* const raw = in.raw;
    if (P < 0 || width <= 0 || height <= 0 || !alloc.geometry || !alloc.binning || !alloc.image) {
        g_last_error = "gsr_forward: invalid size or missing allocator"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!background || !out.color || !out.depth || !out.opacity || !out.n_touched) { g_last_error = "gsr_forward: null output/background"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P > 0 && raw) {
        if (!cam.viewmatrix || !cam.projmatrix || !cam.cam_pos || M <= 0 || !raw_inputs_ok(raw, M)) { g_last_error = "gsr_forward_raw: null / inconsistent input"; return GSR_ERR_INVALID_ARGUMENT; }
        if (D < 0 || D > 3 || (D + 1) * (D + 1) > M) { g_last_error = "gsr_forward_raw: sh degree out of range for M"; return GSR_ERR_INVALID_ARGUMENT; }
    } else if (P > 0) {
        if (!in.means3D || !in.opacities || !cam.viewmatrix || !cam.projmatrix || !cam.cam_pos) { g_last_error = "gsr_forward: null input"; return GSR_ERR_INVALID_ARGUMENT; }
        if (!in.cov3D_precomp && (!in.scales || !in.rotations)) { g_last_error = "gsr_forward: need scales+rotations or cov3D_precomp"; return GSR_ERR_INVALID_ARGUMENT; }
        // rasterizer_impl.cu:245-248 analogue: colours must come from somewhere
        if (!in.colors_precomp && (!in.shs || M <= 0)) { g_last_error = "gsr_forward: need shs (M>0) or colors_precomp"; return GSR_ERR_INVALID_ARGUMENT; }
        if (!in.colors_precomp && (D < 0 || D > 3 || (D + 1) * (D + 1) > M)) { g_last_error = "gsr_forward: sh degree out of range for M"; return GSR_ERR_INVALID_ARGUMENT; }
    }
    const bool flow = raw && raw->flow_proj1;
    const FwdPlan plan = plan_forward(c.opt, P, D, M, width, height, flow, in.colors_precomp != nullptr);
    const int gx = plan.d.gx, gy = plan.d.gy, T = plan.d.T, nblocks = plan.d.nblocks;
    const bool lds_hist = plan.lds_hist, order_items = plan.order_items;
    const size_t N = (size_t)width * height;
    SpecState& spec = *c.spec;
    const int prefiltered = in.prefiltered;

    char* gchunk = alloc.geometry(alloc.geometry_user, gsr_geometry_buffer_size(P));
    char* ichunk = alloc.image(alloc.image_user, gsr_image_buffer_size(width, height, P));
    if (!gchunk || !ichunk) { g_last_error = "gsr_forward: allocation callback returned NULL"; return GSR_ERR_ALLOC; }
    GeomState geom = GeomState::from(gchunk, (size_t)P);
    ImageState img = ImageState::from(ichunk, N, (size_t)T, (size_t)P);
    const int* const flow_clip = flow ? c.flow_clip : nullptr;
    int* const radii = out.radii ? out.radii : geom.internal_radii;   // rasterizer_impl.cu:232-235

    // Zero-filled scratch: the flag word only when someone can raise it (prefiltered; the reference's callers never set it), the
    // per-tile counters only when they are accumulated with atomics (the fallback for frames with more tiles than the LDS
    // histogram holds; otherwise tile_offsets_kernel writes them). The common case needs no memset at all.
    uint32_t* const flags = img.tile_count + (size_t)T * CTR_STRIDE;
    if (!lds_hist)
        GSR_HIP_CHECK(hipMemsetAsync(img.tile_count, 0, ((size_t)T * CTR_STRIDE + 1) * sizeof(uint32_t), stream));
    else if (prefiltered)
        GSR_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));

    if (P > 0) {
        PreprocessArgs a = preprocess_args(plan, D, M, scale_modifier, cam.tan_fovx, cam.tan_fovy, prefiltered, to_device_view(raw, flow_clip));
        a.means3D = in.means3D; a.scales = in.scales; a.rotations = in.rotations; a.opacities = in.opacities;
        a.shs = in.shs; a.cov3D_precomp = in.cov3D_precomp; a.colors_precomp = in.colors_precomp;
        a.viewmatrix = cam.viewmatrix; a.projmatrix = cam.projmatrix; a.cam_pos = cam.cam_pos;
        a.radii = radii; a.n_touched = out.n_touched;
        a.rec = geom.rec; a.cov3D = geom.cov3D;
        a.clamped = geom.clamped; a.tiles_touched = geom.tiles_touched; a.block_sums = geom.block_sums; a.tile_count = img.tile_count;
        a.flags = flags; a.block_tile_base = lds_hist ? img.block_tile_base : nullptr;
        {
            ScopedKernelTimer tm(K_PREPROCESS, stream);
            const int rc = with_raw_pre(raw != nullptr, raw && raw->delta_mode, [&](auto k) {
                return launch_preprocess<preprocess_fwd_kernel<k.raw, k.pre>>(plan, dim3(nblocks), stream, a);
            });
            if (rc) return rc;
        }
        GSR_STAGE("preprocess_fwd");   // (returns the launch's error: hipGetLastError)
        if (lds_hist) {
            ScopedKernelTimer tm(K_SCAN, stream);
            with_tile_offsets(plan, [&](auto s) {      // (tile_cursor: free on this path; holds the dense list lengths)
                hipLaunchKernelGGL((tile_offsets_kernel<s.segs, s.rmax>), dim3((T + TO_COLS - 1) / TO_COLS), dim3(TO_COLS * s.segs), 0, stream, nblocks, T, img.block_tile_base,
                                   img.tile_count, img.tile_cursor);
            });
        }
        GSR_STAGE("tile_offsets");
    } else if (lds_hist) {
        GSR_HIP_CHECK(hipMemsetAsync(img.tile_count, 0, (size_t)T * CTR_STRIDE * sizeof(uint32_t), stream));   // no Gaussians: no columns to scan
    }
    // Speculation: a SLAM loop renders nearly the same scene again and again, so the binning buffer is allocated for what
    // sufficed last time plus slack and scatter / sort / render are enqueued right behind the scan, WITHOUT waiting for R;
    // the host reads R from the mailbox afterwards, while the GPU is already busy with them. The scan kernel compares the
    // frame's real needs with the speculative capacity and raises FLAG_OVERFLOW if they do not fit: the speculative kernels
    // then exit at once and the host redoes them on an exact-size buffer (also the path of the first call and of debug mode).
    if (c.opt.lazy && spec.mailbox) {
        // lazy mode never waits, so the capacity estimate is refreshed from whatever header the GPU published last (a few calls old)
        const uint32_t s0 = __atomic_load_n(&spec.mailbox[4], __ATOMIC_ACQUIRE);
        if (s0 != 0) {
            const uint32_t r = __atomic_load_n(&spec.mailbox[0], __ATOMIC_RELAXED), ra = __atomic_load_n(&spec.mailbox[2], __ATOMIC_RELAXED);
            const uint32_t mx = __atomic_load_n(&spec.mailbox[3], __ATOMIC_RELAXED);
            if (__atomic_load_n(&spec.mailbox[4], __ATOMIC_ACQUIRE) == s0 && r <= 0x7fffffffu && ra <= 0x7fffffffu) {
                const size_t need = ra > r ? ra : r;
                // grow at once, shrink slowly: a view that briefly needs less must not take the slack away from the next one
                spec.last_R_alloc = need > spec.last_R_alloc ? need : spec.last_R_alloc - (spec.last_R_alloc - need) / 16;
                spec.last_max_tile = mx > spec.last_max_tile ? mx : spec.last_max_tile;
            }
        }
    }
    const bool speculate = c.opt.speculate && spec.last_R_alloc && !debug && P > 0;
    const size_t cap = speculate ? spec_capacity(spec.last_R_alloc) : 0;
    const uint32_t cap_tile = tile_list_capacity(spec.last_max_tile);
    // F2b (gs_forward.h): on a speculative frame of the LDS-histogram path the scatter launch does the scan's work itself -- one launch less
    const bool scan_in_scatter = speculate && lds_hist && nblocks <= GB;
    {
        ScopedKernelTimer tm(K_SCAN, stream);
        { const int rc = ensure_mailbox(spec); if (rc) return rc; }
        if (++spec.seq == 0) spec.seq = 1;
        if (!scan_in_scatter)
            hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, stream, nblocks, geom.block_sums, geom.block_base, T, img.tile_count,
                               img.ranges, img.tile_cursor, prefiltered ? flags : (const uint32_t*)nullptr, (uint32_t)cap, cap_tile, img.chunk_base,
                               geom.header,
                               c.opt.mailbox ? spec.mailbox_dev : nullptr, spec.seq);
    }
    GSR_STAGE("scan");

    // render_fwd, or its tracking variant with the loss epilogue (gsr_track_step)
    auto launch_render_fwd = [&](auto... args) {
        ScopedKernelTimer tm(K_RENDER_FWD, stream);
        if (c.track_loss) hipLaunchKernelGGL(render_fwd_track_kernel, dim3(T), dim3(RB), 0, stream, args..., *c.track_loss);
        else hipLaunchKernelGGL(render_fwd_kernel, dim3(T), dim3(RB), 0, stream, args...);
    };
    // scatter -> sort -> render on a binning buffer laid out for carve_R instances / cap_sorted sorted entries
    auto enqueue_binning_and_render = [&](char* chunk, size_t carve_R, size_t cap_sorted, bool spec_launch, bool any_padding,
                                          uint32_t longest_list) -> int {
        const BinningPtrs bin = carve_binning(chunk, carve_R, cap_sorted, (size_t)T);
        uint32_t* const chk = spec_launch ? geom.header : nullptr;
        if (any_padding) GSR_HIP_CHECK(hipMemsetAsync(bin.keys, 0xFF, cap_sorted * sizeof(uint64_t), stream));   // sort padding
        {
            ScopedKernelTimer tm(K_SCATTER, stream);
            ScanInScatter sis{};
            if (spec_launch && scan_in_scatter) {
                sis.dense_total = img.tile_cursor; sis.block_sums = geom.block_sums; sis.nblocks = nblocks; sis.ranges = img.ranges; sis.block_base = geom.block_base;
                sis.chunk_base = img.chunk_base; sis.flags = prefiltered ? flags : (const uint32_t*)nullptr; sis.cap_R = (uint32_t)cap; sis.cap_tile_list = cap_tile;
                sis.host_mailbox = c.opt.mailbox ? spec.mailbox_dev : nullptr; sis.seq = spec.seq;
            }
            hipLaunchKernelGGL(scatter_instances_kernel, dim3(nblocks + (order_items || sis.dense_total ? 1 : 0)), dim3(GB), plan.hist_lds_bytes, stream, P, gx, gy, radii, geom.rec,
                               geom.tiles_touched, geom.block_base, geom.point_offsets, img.tile_cursor, img.ranges,
                               lds_hist ? img.block_tile_base : nullptr, bin.keys, bin.inst_gauss, geom.header, spec_launch ? 1 : 0,
                               (uint32_t)carve_R, (uint32_t)cap_sorted, plan.eager, flow_clip,
                               order_items ? img.tile_count : (uint32_t*)nullptr, plan.order_fwd, sis);
        }
        GSR_STAGE("scatter_instances");
        if (const SortTier tier = sort_tier(longest_list); tier.kind != SortTier::NONE) {
            ScopedKernelTimer tm(K_SORT, stream);
            if (tier.kind == SortTier::MID)
                hipLaunchKernelGGL((sort_tiles_kernel<SORT_MID_CAP, SORT_SMALL_CAP>), dim3(T), dim3(256), 0, stream, T, img.ranges, bin.keys, bin.inst_gauss, bin.sorted, chk);
            else
                hipLaunchKernelGGL((sort_tiles_kernel<SORT_LDS_CAP, SORT_SMALL_CAP>), dim3(T), dim3(256), 0, stream, T, img.ranges, bin.keys, bin.inst_gauss, bin.sorted, chk);
            if (tier.chunks) {
                const dim3 g((unsigned)T, tier.chunks);
                hipLaunchKernelGGL((sort_long_chunks_kernel<SORT_LDS_CAP>), g, dim3(256), 0, stream, img.ranges, bin.keys, chk, (uint32_t)SORT_LDS_CAP);
                hipLaunchKernelGGL((rank_long_chunks_kernel<SORT_LDS_CAP>), g, dim3(256), 0, stream, img.ranges, (const uint64_t*)bin.keys,
                                   (const uint32_t*)bin.inst_gauss, bin.sorted, chk, (uint32_t)SORT_LDS_CAP);
            }
        }
        GSR_STAGE("sort_tiles");
        // Tiles with an empty range still run and write the background (forward.cu:297-299,382-391; Q21).
        launch_render_fwd(T, gx, img.ranges, bin.sorted, width, height, geom.rec, background, img.final_T, img.n_contrib, out.color, out.depth,
                          out.opacity, out.n_touched, img.final_C, bin.ckpt, chk, (const uint64_t*)bin.keys, (const uint32_t*)bin.inst_gauss, bin.sorted,
                          (const uint32_t*)img.chunk_base, bin.chunk_info, order_items ? (const uint32_t*)img.tile_count : (const uint32_t*)nullptr,
                          plan.order_fwd ? 1 : 0);
        GSR_STAGE("render_fwd");
        return 0;
    };

    char* bchunk = nullptr;
    if (speculate) {
        bchunk = alloc.binning(alloc.binning_user, binning_bytes(cap, cap, (size_t)T));
        if (!bchunk) { g_last_error = "gsr_forward: binning allocation callback returned NULL"; return GSR_ERR_ALLOC; }
        const int rc = enqueue_binning_and_render(bchunk, cap, cap, true, false, cap_tile);
        if (rc) return rc;
    }
    if (speculate && c.opt.lazy) return (int)(cap > 0x7fffffffull ? 0x7fffffffull : cap);   // no wait: see t_lazy
    // The one host wait of the forward pass (the reference's is the blocking cudaMemcpy at rasterizer_impl.cu:283-284).
    uint32_t hdr[4];
    { const int rc = wait_for_header(stream, spec, c.opt.mailbox, geom.header, spec.seq, hdr); if (rc) return rc; }
    if (hdr[HDR_FLAGS] & FLAG_PREFILTERED) { g_last_error = "Point is filtered although prefiltered is set. This shouldn't happen!"; return GSR_ERR_PREFILTERED; }
    FrameCounts f;
    { const int rc = absorb_header(spec, hdr, "gsr_forward", f); if (rc) return rc; }
    const uint32_t R = f.R, R_alloc = f.R_alloc;
    if (speculate && !(f.flags & FLAG_OVERFLOW)) return (int)R;

    if (R > 0) {
        bchunk = alloc.binning(alloc.binning_user, binning_bytes((size_t)R, (size_t)R_alloc, (size_t)T));
        if (!bchunk) { g_last_error = "gsr_forward: binning allocation callback returned NULL"; return GSR_ERR_ALLOC; }
        const int rc = enqueue_binning_and_render(bchunk, (size_t)R, (size_t)R_alloc, false, R_alloc != R, f.max_tile);
        if (rc) return rc;
    } else {
        if (!bchunk) bchunk = alloc.binning(alloc.binning_user, binning_bytes(0, 0, (size_t)T));
        if (!bchunk) { g_last_error = "gsr_forward: binning allocation callback returned NULL"; return GSR_ERR_ALLOC; }
        // keep point_offsets defined for debug readers / backward even when nothing is visible
        if (P > 0) GSR_HIP_CHECK(hipMemsetAsync(geom.point_offsets, 0, (size_t)P * sizeof(uint32_t), stream));
        launch_render_fwd(T, gx, img.ranges, (const uint2*)nullptr, width, height, geom.rec, background, img.final_T, img.n_contrib, out.color,
                          out.depth, out.opacity, out.n_touched, img.final_C, (float*)nullptr, (const uint32_t*)nullptr,
                          (const uint64_t*)nullptr, (const uint32_t*)nullptr, (uint2*)nullptr, (const uint32_t*)nullptr, (uint4*)nullptr,
                          (const uint32_t*)nullptr, 0);
    }
    GSR_STAGE("render_fwd");
    return (int)R;
}

extern "C" {

int gsr_forward(gsr_alloc_fn geometry_alloc, void* geometry_user, gsr_alloc_fn binning_alloc, void* binning_user,
                gsr_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width, int height,
                const float* means3D, const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                float* out_depth, float* out_opacity, int* radii, int* n_touched, int debug, void* stream)
{
    Call c{read_options(), &spec_state(0)};
    const FwdInputs in{means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, prefiltered, nullptr};
    return forward_impl(c, {geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user}, P, D, M, background, width, height,
                        in, scale_modifier, {viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy}, {out_color, out_depth, out_opacity, radii, n_touched},
                        debug, stream);
}

int gsr_forward_raw(gsr_alloc_fn geometry_alloc, void* geometry_user, gsr_alloc_fn binning_alloc, void* binning_user,
                    gsr_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width, int height,
                    const gsr_raw_inputs* in, float scale_modifier, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                    float tan_fovx, float tan_fovy, float* out_color, float* out_depth, float* out_opacity, int* radii, int* n_touched,
                    int debug, void* stream)
{
    if (!in) { g_last_error = "gsr_forward_raw: null input descriptor"; return GSR_ERR_INVALID_ARGUMENT; }
    Call c{read_options(), &spec_state(0)};
    FwdInputs fin;
    fin.raw = in;
    return forward_impl(c, {geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user}, P, D, M, background, width, height,
                        fin, scale_modifier, {viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy}, {out_color, out_depth, out_opacity, radii, n_touched},
                        debug, stream);
}

}  // extern "C"

// ---- multi-view entry point (include/gs_rasterizer.h, csrc/gs_views.h) ------------------------------------------------------------------
namespace {
struct CapturedAlloc { gsr_alloc_fn fn; void* user; char* got; };
char* captured_alloc(void* u, size_t bytes)
{
    CapturedAlloc* c = static_cast<CapturedAlloc*>(u);
    c->got = c->fn(c->user, bytes);
    return c->got;
}
// the three allocations of one forward pass, remembered for the caller
struct CapturedAllocs {
    CapturedAlloc g, b, i;
    FwdAllocs fns() { return {captured_alloc, &g, captured_alloc, &b, captured_alloc, &i}; }
};
}  // namespace

extern "C" int gsr_forward_views(int V, gsr_view* views, gsr_alloc_fn geometry_alloc, gsr_alloc_fn binning_alloc, gsr_alloc_fn image_alloc, int P, int D, int M,
                                 const float* background, int width, int height, const gsr_raw_inputs* in, float scale_modifier, float tan_fovx,
                                 float tan_fovy, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || V > MAX_VIEWS || !views || !in || P <= 0 || width <= 0 || height <= 0 || !geometry_alloc || !binning_alloc || !image_alloc || !background ||
        M <= 0 || D < 0 || D > 3 || (D + 1) * (D + 1) > M || in->gather || in->flow_proj1) {
        g_last_error = "gsr_forward_views: invalid argument (1 <= V <= GSR_MAX_VIEWS, P > 0, raw inputs without gather; flow mode is per view)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const bool flow = views[0].flow_proj1 != nullptr;      // render_flow views: every view of the call, or none
    for (int v = 0; v < V; v++) {
        const gsr_view& w = views[v];
        const gsr_raw_inputs probe = view_raw_inputs(*in, w);
        if (!w.viewmatrix || !w.projmatrix || !w.cam_pos || !w.out_color || !w.out_depth || !w.out_opacity || !w.radii || !w.n_touched ||
            (w.flow_proj1 != nullptr) != flow || !raw_inputs_ok(&probe, M)) {
            g_last_error = "gsr_forward_views: null / inconsistent view descriptor"; return GSR_ERR_INVALID_ARGUMENT;
        }
    }
    // flow batches keep their own capacity estimates (their v-th view is another camera), and so does every call of an iteration that needs
    // several (view_slot_group): a slot shared by two calls per iteration sees its estimate flip between two cameras -- eager calls then redo
    // the view through the single-view path every time, captured ones overflow at every replay
    const int slot0 = 1 + t_view_slot_group * 2 * MAX_VIEWS + (flow ? MAX_VIEWS : 0);
    Options opt = read_options();
    auto forward_one_view = [&](const Options& o, int v) -> int {   // view v through the single-view path, on its view slot
        gsr_view& vw = views[v];
        const gsr_raw_inputs one = view_raw_inputs(*in, vw);
        Call c{o, &spec_state(slot0 + v), vw.flow_clip};
        FwdInputs fin;
        fin.raw = &one;
        CapturedAllocs al{{geometry_alloc, vw.geometry_user, nullptr}, {binning_alloc, vw.binning_user, nullptr}, {image_alloc, vw.image_user, nullptr}};
        const int rc = forward_impl(c, al.fns(), P, D, M, background, width, height, fin, scale_modifier, {vw.viewmatrix, vw.projmatrix, vw.cam_pos, tan_fovx, tan_fovy},
                                    {vw.out_color, vw.out_depth, vw.out_opacity, vw.radii, vw.n_touched}, debug, stream_);
        if (rc < 0) return rc;
        vw.geom_buffer = al.g.got; vw.binning_buffer = al.b.got; vw.image_buffer = al.i.got; vw.num_rendered = rc;
        return 0;
    };
    const FwdPlan plan = plan_forward(opt, P, D, M, width, height, flow, false);
    const ViewDims& d = plan.d;
    // the batched path needs a capacity estimate for every slot (the first iteration of a window goes view by view and leaves one)
    bool batched = !debug && opt.speculate && plan.lds_hist && V > 1;
    for (int v = 0; v < V && batched; v++) batched = spec_state(slot0 + v).last_R_alloc != 0;
    if (!batched) {
        for (int v = 0; v < V; v++) {
            const int rc = forward_one_view(opt, v);
            if (rc) return rc;
        }
        return 0;
    }
    t_views_batched++;
    ViewTable t;
    memset(&t, 0, sizeof(t));
    uint32_t last_max_tile = 0;
    for (int v = 0; v < V; v++) last_max_tile = std::max(last_max_tile, spec_state(slot0 + v).last_max_tile);
    const uint32_t cap_tile = tile_list_capacity(last_max_tile);
    for (int v = 0; v < V; v++) {
        gsr_view& w = views[v];
        SpecState& spec = spec_state(slot0 + v);
        { const int rc = ensure_mailbox(spec); if (rc) return rc; }
        if (++spec.seq == 0) spec.seq = 1;
        const size_t cap = spec_capacity(spec.last_R_alloc);
        w.geom_buffer = geometry_alloc(w.geometry_user, gsr_geometry_buffer_size(P));
        w.image_buffer = image_alloc(w.image_user, gsr_image_buffer_size(width, height, P));
        w.binning_buffer = binning_alloc(w.binning_user, binning_bytes(cap, cap, (size_t)d.T));
        if (!w.geom_buffer || !w.image_buffer || !w.binning_buffer) { g_last_error = "gsr_forward_views: allocation callback returned NULL"; return GSR_ERR_ALLOC; }
        ViewSlot& s = t.v[v];
        fill_view_slot(s, w);
        s.flow_clip = flow ? w.flow_clip : nullptr;
        s.out_color = w.out_color; s.out_depth = w.out_depth; s.out_opacity = w.out_opacity; s.n_touched = w.n_touched;
        s.mailbox = opt.mailbox ? spec.mailbox_dev : nullptr; s.cap = (uint32_t)std::min<size_t>(cap, 0x7fffffffu); s.cap_tile = cap_tile; s.seq = spec.seq;
    }
    const PreprocessArgs a = preprocess_args(plan, D, M, scale_modifier, tan_fovx, tan_fovy, 0, to_device_view(in, nullptr));
    const dim3 gv((unsigned)d.nblocks, (unsigned)V), tv((unsigned)d.T, (unsigned)V);
    {
        ScopedKernelTimer tm(K_PREPROCESS, stream);
        const int rc = with_raw_pre<true>(true, in->delta_mode, [&](auto k) {
            return launch_preprocess<preprocess_views_kernel<k.raw, k.pre>>(plan, gv, stream, a, t, d);
        });
        if (rc) return rc;
    }
    {
        ScopedKernelTimer tm(K_SCAN, stream);
        with_tile_offsets(plan, [&](auto s) {
            hipLaunchKernelGGL((tile_offsets_views_kernel<s.segs, s.rmax>), dim3((unsigned)((d.T + TO_COLS - 1) / TO_COLS), (unsigned)V), dim3(TO_COLS * s.segs), 0, stream, t, d);
        });
        hipLaunchKernelGGL(scan_views_kernel, dim3(1, (unsigned)V), dim3(1024), 0, stream, t, d);
    }
    {
        ScopedKernelTimer tm(K_SCATTER, stream);
        hipLaunchKernelGGL(scatter_views_kernel, dim3((unsigned)d.nblocks + (plan.order_items ? 1u : 0u), (unsigned)V), dim3(GB), plan.hist_lds_bytes, stream, t, d, plan.eager,
                           plan.order_word);
    }
    if (const SortTier tier = sort_tier(cap_tile); tier.kind != SortTier::NONE) {
        ScopedKernelTimer tm(K_SORT, stream);
        if (tier.kind == SortTier::MID) hipLaunchKernelGGL((sort_tiles_views_kernel<SORT_MID_CAP, SORT_SMALL_CAP>), tv, dim3(256), 0, stream, t, d);
        else hipLaunchKernelGGL((sort_tiles_views_kernel<SORT_LDS_CAP, SORT_SMALL_CAP>), tv, dim3(256), 0, stream, t, d);
        if (tier.chunks) {
            const dim3 gl((unsigned)d.T, tier.chunks, (unsigned)V);
            hipLaunchKernelGGL((sort_long_chunks_views_kernel<SORT_LDS_CAP>), gl, dim3(256), 0, stream, t, d, (uint32_t)SORT_LDS_CAP);
            hipLaunchKernelGGL((rank_long_chunks_views_kernel<SORT_LDS_CAP>), gl, dim3(256), 0, stream, t, d, (uint32_t)SORT_LDS_CAP);
        }
    }
    {
        ScopedKernelTimer tm(K_RENDER_FWD, stream);
        hipLaunchKernelGGL(render_fwd_views_kernel, tv, dim3(RB), 0, stream, t, d, background, 1, plan.order_word);
    }
    GSR_HIP_CHECK(hipGetLastError());
    // one wait per view (they are all long done by the time the host has enqueued the tile kernels); a view that outgrew its capacity is
    // redone through the single-view path, which allocates exactly
    for (int v = 0; v < V; v++) {
        gsr_view& w = views[v];
        SpecState& spec = spec_state(slot0 + v);
        if (opt.lazy) { w.num_rendered = (int)t.v[v].cap; continue; }
        uint32_t hdr[4];
        char* gp = w.geom_buffer;
        const GeomState geom = GeomState::from(gp, (size_t)P);
        { const int rc = wait_for_header(stream, spec, opt.mailbox, geom.header, t.v[v].seq, hdr); if (rc) return rc; }
        FrameCounts f;
        { const int rc = absorb_header(spec, hdr, "gsr_forward_views", f); if (rc) return rc; }
        w.num_rendered = (int)f.R;
        if (f.flags & FLAG_OVERFLOW) {
            // (without speculation: the counts are known, the redo is laid out for exactly them. A speculative redo would overflow a
            // second time under "cap_test_shrink_permille" and count the same frame twice in the sticky overflow counter.)
            Options exact = opt;
            exact.speculate = false;
            const int rc = forward_one_view(exact, v);
            if (rc) return rc;
        }
    }
    return 0;
}

// scratch of gsr_backward_views: per view one row of partial gradients (PartLayout), each row starting on a multiple of 256 bytes
struct ViewsScratch { float* part; size_t row_floats, bytes; };
static ViewsScratch views_scratch_layout(int V, int P, int M, int scale_dim, const char* scratch)
{
    Carver c(scratch, 256, true);
    const size_t row_floats = V > 0 && P > 0 ? c.up(part_layout((size_t)P, M, scale_dim).total * sizeof(float)) / sizeof(float) : 0;
    return {c.take<float>((size_t)std::max(V, 0) * row_floats), row_floats, c.bytes()};
}

extern "C" size_t gsr_views_scratch_size(int V, int P, int M, int scale_dim) { return views_scratch_layout(V, P, M, scale_dim, nullptr).bytes; }

extern "C" int gsr_backward_views(int V, gsr_view* views, int P, int D, int M, const float* background, int width, int height, const gsr_raw_inputs* in,
                                  float scale_modifier, float tan_fovx, float tan_fovy, const gsr_raw_grads* out, char* scratch, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const bool accumulate = (debug & GSR_BACKWARD_ACCUMULATE) != 0, pose_only = (debug & GSR_BACKWARD_POSE_ONLY) != 0;
    const bool flow = views && V >= 1 && views[0].flow_proj1 != nullptr;      // flow views: only out->xyz is required (constants otherwise, :307,326-334)
    if (V < 1 || V > MAX_VIEWS || !views || !in || P <= 0 || width <= 0 || height <= 0 || !background || in->gather || in->flow_proj1 ||
        (!pose_only && (!out || !scratch || !out->xyz ||
                        (!flow && (!out->log_scales || !out->raw_rotations || !out->logit_opacity || !out->features_dc || (M > 1 && !out->features_rest)))))) {
        g_last_error = "gsr_backward_views: invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const Options opt = read_options();
    const ViewDims d = view_dims(P, width, height);
    ViewTable t;
    memset(&t, 0, sizeof(t));
    const ViewsScratch sc = views_scratch_layout(V, P, M, in->scale_dim, scratch);
    int max_R = 0;
    for (int v = 0; v < V; v++) {
        const gsr_view& w = views[v];
        if (!w.geom_buffer || !w.binning_buffer || !w.image_buffer || !w.dL_dcolor || !w.dL_ddepth || !w.dL_dmean2D || !w.viewmatrix || !w.projmatrix ||
            !w.projmatrix_raw || !w.cam_pos || !w.radii || (w.flow_proj1 != nullptr) != flow || (flow && !w.flow_proj2)) {
            g_last_error = "gsr_backward_views: null / inconsistent view argument"; return GSR_ERR_INVALID_ARGUMENT;
        }
        ViewSlot& s = t.v[v];
        fill_view_slot(s, w);
        s.ddx2 = w.ddx2;
        s.dL_dpix = w.dL_dcolor; s.dL_dpix_depth = w.dL_ddepth; s.dL_dmean2D = w.dL_dmean2D; s.ddx = w.ddx; s.dds = w.dds; s.ddr = w.ddr; s.tau_sum = w.dL_dtau_sum;
        s.part = pose_only ? nullptr : sc.part + (size_t)v * sc.row_floats;
        s.cap = (uint32_t)std::max(0, w.num_rendered);
        max_R = std::max(max_R, w.num_rendered);
    }
    {
        ScopedKernelTimer tm(K_RENDER_BWD, stream);
        if (max_R > 0) {
            hipLaunchKernelGGL(render_bwd_views_kernel, dim3((unsigned)(max_R / CHUNK + d.T), (unsigned)V), dim3(RB), 0, stream, t, d, background);
        }
    }
    const GeomBwdArgs a = geom_bwd_args(opt, d, D, M, scale_modifier, tan_fovx, tan_fovy, pose_only, to_device_view(in, nullptr), in->scale_dim);
    {
        ScopedKernelTimer tm(K_GEOM_BWD, stream);
        with_raw_pre<true>(true, in->delta_mode, [&](auto k) {
            hipLaunchKernelGGL((geometry_bwd_views_kernel<k.raw, k.pre>), dim3((unsigned)((P + 255) / 256), (unsigned)V), dim3(256), 0, stream, a, t, d);
        });
        hipLaunchKernelGGL(tau_sum_views_kernel, dim3(1, (unsigned)V), dim3(384), 0, stream, t, d);
        if (!pose_only) {
            ReduceTargets r{out->xyz, out->features_dc, out->features_rest, out->logit_opacity, out->log_scales, out->raw_rotations};
            hipLaunchKernelGGL(views_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, V, t, P, M, in->scale_dim, r, accumulate ? 1 : 0);
        }
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static int backward_impl(const Call& c, int P, int D, int M, const float* background, int width, int height, const FwdInputs& in, float scale_modifier,
                         const FwdCamera& cam, const BwdState& st, const BwdCotangents& ct, const BwdGrads& g, const gsr_raw_grads* rawg, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const gsr_raw_inputs* const raw = in.raw;
    const bool accumulate = (debug & GSR_BACKWARD_ACCUMULATE) != 0;     // include/gs_rasterizer.h
    const bool pose_only = (debug & GSR_BACKWARD_POSE_ONLY) != 0;
    debug &= 1;
    if (P < 0 || st.R < 0 || width <= 0 || height <= 0) { g_last_error = "gsr_backward: invalid size"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P == 0) { if (g.dL_dtau_sum) GSR_HIP_CHECK(hipMemsetAsync(g.dL_dtau_sum, 0, 6 * sizeof(float), stream)); return 0; }
    if (!st.geom_buffer || !st.binning_buffer || !st.image_buffer || !ct.dL_dpix || !ct.dL_dpix_depth || !background || (!in.means3D && !raw) || !cam.viewmatrix ||
        !cam.projmatrix || !cam.projmatrix_raw || !cam.cam_pos || !g.dL_dmean2D || (!pose_only && (!g.dL_dopacity || !g.dL_dmean3D)) || (!g.dL_dtau && !g.dL_dtau_sum) ||
        (raw && (!raw_inputs_ok(raw, M) || !rawg ||
                 (!pose_only && (!g.dL_dscale || !g.dL_drot || (!raw->flow_proj1 && (!rawg->features_dc || (M > 1 && !rawg->features_rest)))))))) {
        g_last_error = "gsr_backward: null argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const ViewDims d = view_dims(P, width, height);
    char* gp = st.geom_buffer; char* ip = st.image_buffer;
    GeomState geom = GeomState::from(gp, (size_t)P);
    ImageState img = ImageState::from(ip, (size_t)width * height, (size_t)d.T, 0);
    if (st.R > 0) {
        // one block per CHUNK entries of a tile list; sum over tiles of ceil(n / CHUNK) <= R / CHUNK + T, surplus blocks exit
        ScopedKernelTimer tm(K_RENDER_BWD, stream);
        const int grid = st.R / CHUNK + d.T;
        hipLaunchKernelGGL(render_bwd_kernel, dim3(grid), dim3(RB), 0, stream, d.T, d.gx, (const char*)st.binning_buffer,
                           (const uint32_t*)geom.header, width, height, background, geom.rec,
                           img.final_T, img.final_C, img.n_contrib, ct.dL_dpix, ct.dL_dpix_depth);
    }
    GSR_STAGE("render_bwd");
    GeomBwdArgs a = geom_bwd_args(c.opt, d, D, M, scale_modifier, cam.tan_fovx, cam.tan_fovy, pose_only, to_device_view(raw, nullptr), raw ? raw->scale_dim : 0);
    a.means3D = in.means3D; a.shs = in.shs; a.clamped = geom.clamped; a.scales = in.scales; a.rotations = in.rotations;
    a.radii = st.radii ? st.radii : geom.internal_radii;                       // rasterizer_impl.cu:387-390
    a.cov3Ds = in.cov3D_precomp ? in.cov3D_precomp : geom.cov3D;               // rasterizer_impl.cu:429
    a.viewmatrix = cam.viewmatrix; a.projmatrix = cam.projmatrix; a.projmatrix_raw = cam.projmatrix_raw; a.campos = cam.cam_pos;
    a.tiles_touched = geom.tiles_touched; a.point_offsets = geom.point_offsets; a.bin_base = st.binning_buffer; a.header = geom.header;
    a.dL_dmean2D = g.dL_dmean2D; a.dL_dconic = g.dL_dconic; a.dL_dopacity = g.dL_dopacity; a.dL_dcolor = g.dL_dcolor; a.dL_ddepth = g.dL_ddepth;
    a.dL_dmean3D = g.dL_dmean3D; a.dL_dcov3D = g.dL_dcov3D; a.dL_dsh = g.dL_dsh; a.dL_dscale = g.dL_dscale; a.dL_drot = g.dL_drot; a.dL_dtau = g.dL_dtau;
    a.accumulate = accumulate ? 1 : 0;
    a.tau_partials = g.dL_dtau_sum ? geom.tau_partials : nullptr;
    if (raw) { a.rawg.f_dc = rawg->features_dc; a.rawg.f_rest = rawg->features_rest; a.rawg.ddx = rawg->dx; a.rawg.dds = rawg->ds; a.rawg.ddr = rawg->dr; a.rawg.ddx2 = rawg->dx2; }
    {
        ScopedKernelTimer tm(K_GEOM_BWD, stream);
        with_raw_pre(raw != nullptr, raw && raw->delta_mode, [&](auto k) {
            hipLaunchKernelGGL((geometry_bwd_kernel<k.raw, k.pre>), dim3((P + 255) / 256), dim3(256), 0, stream, a);
        });
        if (g.dL_dtau_sum && c.track_tail)     // gsr_track_step: pose-gradient sum + exposure-gradient sum + camera step in one launch
            hipLaunchKernelGGL(track_tail_kernel, dim3(1), dim3(384), 0, stream, (P + 255) / 256, (const float*)geom.tau_partials, g.dL_dtau_sum, d.T,
                               c.track_tail->exposure_partials, c.track_tail->dL_dexposure, c.track_tail->step);
        else if (g.dL_dtau_sum)
            hipLaunchKernelGGL(tau_sum_kernel, dim3(1), dim3(384), 0, stream, (P + 255) / 256, geom.tau_partials, g.dL_dtau_sum);
    }
    GSR_STAGE("geometry_bwd");
    return 0;
}

// ---- HexPlane feature field (include/deformation_field.h) -------------------------------------------------------------------
static int hexplane_check(const gsr_hexplane_field* f, int64_t n, const float* xyz, const float* time, const char* who)
{
    auto fail = [&](const char* what) { g_last_error = std::string(who) + ": " + what; return GSR_ERR_INVALID_ARGUMENT; };
    if (!f) return fail("null field descriptor");
    if (n < 0) return fail("negative point count");
    if (f->num_levels < 1 || f->num_levels > GSR_HEXPLANE_MAX_LEVELS) return fail("num_levels outside 1..8");
    if (f->feat_dim != 8 && f->feat_dim != 16 && f->feat_dim != 32 && f->feat_dim != 64) return fail("feat_dim must be 8, 16, 32 or 64");
    for (int l = 0; l < f->num_levels; l++) {
        for (int k = 0; k < 4; k++) if (f->levels[l].res[k] < 1) return fail("resolution < 1");
        for (int p = 0; p < 6; p++) if (!f->levels[l].planes[p]) return fail("null plane");
    }
    if (n > 0 && (!xyz || !time)) return fail("null xyz / time");
    return 0;
}

template <bool BWD, typename... Args>
static void hexplane_launch(const gsr_hexplane_field& f, int64_t n, hipStream_t stream, Args... args)
{
    const int lpp = f.feat_dim / 4;
    if constexpr (BWD) {   // channels-last planes: one channel per lane, a whole texel per atomic instruction (gs_hexplane.h)
        if (f.channels_last) {
            const int ppb = HEX_BLOCK / f.feat_dim;
            const dim3 g((unsigned)((n + ppb - 1) / ppb)), b(HEX_BLOCK);
            switch (f.feat_dim) {
            case 8: hipLaunchKernelGGL((hexplane_bwd_lane_kernel<8>), g, b, 0, stream, f, n, args...); break;
            case 16: hipLaunchKernelGGL((hexplane_bwd_lane_kernel<16>), g, b, 0, stream, f, n, args...); break;
            case 32: hipLaunchKernelGGL((hexplane_bwd_lane_kernel<32>), g, b, 0, stream, f, n, args...); break;
            case 64: hipLaunchKernelGGL((hexplane_bwd_lane_kernel<64>), g, b, 0, stream, f, n, args...); break;
            }
            return;
        }
    }
    const dim3 grid((unsigned)((n + HEX_BLOCK / lpp - 1) / (HEX_BLOCK / lpp))), block(HEX_BLOCK);
#define GSR_HEX_CASE(LPP)                                                                                                       \
    case LPP:                                                                                                                   \
        if constexpr (BWD) { if (f.channels_last) hipLaunchKernelGGL((hexplane_bwd_kernel<LPP, HEX_VEC>), grid, block, 0, stream, f, n, args...);   \
                   else hipLaunchKernelGGL((hexplane_bwd_kernel<LPP, HEX_PLANAR>), grid, block, 0, stream, f, n, args...); }        \
        else     { if (f.channels_last) hipLaunchKernelGGL((hexplane_fwd_kernel<LPP, HEX_VEC>), grid, block, 0, stream, f, n, args...);   \
                   else hipLaunchKernelGGL((hexplane_fwd_kernel<LPP, HEX_PLANAR>), grid, block, 0, stream, f, n, args...); }        \
        break;
    switch (lpp) { GSR_HEX_CASE(2) GSR_HEX_CASE(4) GSR_HEX_CASE(8) GSR_HEX_CASE(16) }
#undef GSR_HEX_CASE
}

extern "C" {

int gsr_backward_fused(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* projmatrix_raw,
                 const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer,
                 char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D, float* dL_dconic,
                 float* dL_dopacity, float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                 float* dL_dscale, float* dL_drot, float* dL_dtau, float* dL_dtau_sum, int debug, void* stream)
{
    FwdInputs in;
    in.means3D = means3D; in.shs = shs; in.colors_precomp = colors_precomp; in.scales = scales; in.rotations = rotations; in.cov3D_precomp = cov3D_precomp;
    BwdGrads g;
    g.dL_dmean2D = dL_dmean2D; g.dL_dconic = dL_dconic; g.dL_dopacity = dL_dopacity; g.dL_dcolor = dL_dcolor; g.dL_ddepth = dL_ddepth; g.dL_dmean3D = dL_dmean3D;
    g.dL_dcov3D = dL_dcov3D; g.dL_dsh = dL_dsh; g.dL_dscale = dL_dscale; g.dL_drot = dL_drot; g.dL_dtau = dL_dtau; g.dL_dtau_sum = dL_dtau_sum;
    return backward_impl(Call{read_options()}, P, D, M, background, width, height, in, scale_modifier, {viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, projmatrix_raw},
                         {geom_buffer, binning_buffer, image_buffer, radii, R}, {dL_dpix, dL_dpix_depth}, g, nullptr, debug, stream);
}

int gsr_backward_raw(int P, int D, int M, int R, const float* background, int width, int height, const gsr_raw_inputs* in,
                     float scale_modifier, const float* viewmatrix, const float* projmatrix, const float* projmatrix_raw,
                     const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer,
                     char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D, const gsr_raw_grads* out,
                     float* dL_dtau_sum, int debug, void* stream)
{
    if (!in || !out) { g_last_error = "gsr_backward_raw: null descriptor"; return GSR_ERR_INVALID_ARGUMENT; }
    FwdInputs fin;
    fin.raw = in;
    BwdGrads g;
    g.dL_dmean2D = dL_dmean2D; g.dL_dopacity = out->logit_opacity; g.dL_dmean3D = out->xyz; g.dL_dscale = out->log_scales; g.dL_drot = out->raw_rotations; g.dL_dtau_sum = dL_dtau_sum;
    return backward_impl(Call{read_options()}, P, D, M, background, width, height, fin, scale_modifier, {viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, projmatrix_raw},
                         {geom_buffer, binning_buffer, image_buffer, radii, R}, {dL_dpix, dL_dpix_depth}, g, out, debug, stream);
}

int gsr_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* projmatrix_raw,
                 const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer,
                 char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D, float* dL_dconic,
                 float* dL_dopacity, float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                 float* dL_dscale, float* dL_drot, float* dL_dtau, int debug, void* stream)
{
    if (P > 0 && (!dL_dconic || !dL_dcolor || !dL_ddepth || !dL_dcov3D || !dL_dtau)) { g_last_error = "gsr_backward: null argument"; return GSR_ERR_INVALID_ARGUMENT; }
    return gsr_backward_fused(P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier, rotations,
                              cov3D_precomp, viewmatrix, projmatrix, projmatrix_raw, campos, tan_fovx, tan_fovy, radii, geom_buffer,
                              binning_buffer, image_buffer, dL_dpix, dL_dpix_depth, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth,
                              dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, dL_dtau, nullptr, debug, stream);
}

#if GSR_TIMELINE
// dev builds only (-DGSR_TIMELINE=1): {start, end (100 MHz ticks), HW_ID, XCC_ID} of every block of the last render_fwd (which = 0, by tile) /
// render_bwd (which = 1, by block) launch
int gsr_debug_spans(unsigned int* out, int nwords, int which)
{
    GSR_HIP_CHECK(hipDeviceSynchronize());
    GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_spans), (size_t)nwords * sizeof(uint32_t), (size_t)which * 8192 * 4 * sizeof(uint32_t)));
    return 0;
}
#endif
#if GSR_FWD_TIMING
// dev builds only (-DGSR_FWD_TIMING=1): per-wave cycle accounting of the last render_fwd launch, 8 words per (tile, quadrant wave)
int gsr_debug_fwd_timing(unsigned int* out, int nwords)
{
    GSR_HIP_CHECK(hipDeviceSynchronize());
    GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fwd_timing), (size_t)nwords * sizeof(uint32_t)));
    return 0;
}
int gsr_debug_pre_timing(unsigned int* out, int nwords, int which)
{
    GSR_HIP_CHECK(hipDeviceSynchronize());
    if (which == 0) GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pre_timing), (size_t)nwords * sizeof(uint32_t)));
    else GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sca_timing), (size_t)nwords * sizeof(uint32_t)));
    return 0;
}
int gsr_debug_geo_timing(unsigned int* out, int nwords)
{
    GSR_HIP_CHECK(hipDeviceSynchronize());
    GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_geo_timing), (size_t)nwords * sizeof(uint32_t)));
    return 0;
}
int gsr_debug_bwd_timing(unsigned int* out, int nwords)
{
    GSR_HIP_CHECK(hipDeviceSynchronize());
    GSR_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_timing), (size_t)nwords * sizeof(uint32_t)));
    return 0;
}
#endif
int gsr_debug_read_state(int P, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                         const char* image_buffer, float* depths, float* means2D, float* conic_opacity, float* rgb, float* cov3D,
                         unsigned char* clamped, uint32_t* tiles_touched, uint32_t* point_offsets, float* final_T, uint32_t* n_contrib,
                         uint32_t* ranges, uint32_t* point_list, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    GSR_HIP_CHECK(hipStreamSynchronize(stream));
    const int gx = (width + TILE_X - 1) / TILE_X, gy = (height + TILE_Y - 1) / TILE_Y, T = gx * gy;
    const size_t N = (size_t)width * height;
    char* gp = const_cast<char*>(geom_buffer); char* bp = const_cast<char*>(binning_buffer); char* ip = const_cast<char*>(image_buffer);
    GeomState geom = GeomState::from(gp, (size_t)P);
    ImageState img = ImageState::from(ip, N, (size_t)T, 0);
    uint32_t hdr[HDR_WORDS] = {0};
    if (P > 0) GSR_HIP_CHECK(hipMemcpy(hdr, geom.header, sizeof(hdr), hipMemcpyDeviceToHost));
    const BinningPtrs bin = carve_binning(bp, hdr[HDR_CARVE_R], hdr[HDR_CAP_SORTED], (size_t)T);
#define D2H(dst, src, bytes) do { if ((dst) && (bytes)) GSR_HIP_CHECK(hipMemcpy((dst), (src), (bytes), hipMemcpyDeviceToHost)); } while (0)
    if (P && (depths || means2D || conic_opacity || rgb)) {   // the packed per-Gaussian rows, handed out in the reference's four arrays
        std::vector<TileRec> rows((size_t)P);
        GSR_HIP_CHECK(hipMemcpy(rows.data(), geom.rec, (size_t)P * sizeof(TileRec), hipMemcpyDeviceToHost));
        for (int i = 0; i < P; i++) {
            const TileRec& r = rows[i];
            if (depths) depths[i] = r.q0.z;
            if (means2D) { means2D[2 * i] = r.q0.x; means2D[2 * i + 1] = r.q0.y; }
            if (conic_opacity) { conic_opacity[4 * i] = r.q1.x; conic_opacity[4 * i + 1] = r.q1.y; conic_opacity[4 * i + 2] = r.q1.z; conic_opacity[4 * i + 3] = r.q0.w; }
            if (rgb) { rgb[3 * i] = r.q2.x; rgb[3 * i + 1] = r.q2.y; rgb[3 * i + 2] = r.q2.z; }
        }
    }
    D2H(cov3D, geom.cov3D, P * 6 * sizeof(float));
    if (clamped && P) {
        std::vector<uint8_t> bits(P);
        GSR_HIP_CHECK(hipMemcpy(bits.data(), geom.clamped, P, hipMemcpyDeviceToHost));
        for (int i = 0; i < P; i++) for (int k = 0; k < 3; k++) clamped[3 * i + k] = (bits[i] >> k) & 1;
    }
    D2H(tiles_touched, geom.tiles_touched, P * sizeof(uint32_t));
    D2H(point_offsets, geom.point_offsets, P * sizeof(uint32_t));
    D2H(final_T, img.final_T, N * sizeof(float));
    D2H(n_contrib, img.n_contrib, N * sizeof(uint32_t));
    std::vector<uint32_t> rg((size_t)T * 2);
    GSR_HIP_CHECK(hipMemcpy(rg.data(), img.ranges, (size_t)T * 8, hipMemcpyDeviceToHost));
    // Padded segments (huge tiles) are compacted so the caller sees the reference's packed layout.
    std::vector<uint32_t> packed((size_t)T * 2);
    uint32_t run = 0, maxend = 0;
    for (int t = 0; t < T; t++) {
        const uint32_t n = rg[2 * t + 1] - rg[2 * t];
        packed[2 * t] = n ? run : 0; packed[2 * t + 1] = n ? run + n : 0;   // empty tiles stay (0,0) like the memset at rasterizer_impl.cu:313
        run += n;
        if (rg[2 * t + 1] > maxend) maxend = rg[2 * t + 1];
    }
    if (ranges) memcpy(ranges, packed.data(), (size_t)T * 8);
    if (point_list && R > 0) {
        std::vector<uint2> srt(maxend);
        GSR_HIP_CHECK(hipMemcpy(srt.data(), bin.sorted, (size_t)maxend * sizeof(uint2), hipMemcpyDeviceToHost));
        size_t o = 0;
        for (int t = 0; t < T; t++)
            for (uint32_t k = rg[2 * t]; k < rg[2 * t + 1]; k++) point_list[o++] = srt[k].x;
    }
#undef D2H
    return 0;
}


// ---- simple_knn.h ---------------------------------------------------------------------------------------------------
struct KnnWorkspace {
    KnnGrid* grid; uint32_t* cell_of; uint32_t* cell_count; uint32_t* cell_start; uint32_t* cursor; float4* sorted_pts;
    size_t bytes;
    static KnnWorkspace from(const char* workspace, size_t P, size_t C)
    {
        Carver c(workspace, 256, true);
        KnnWorkspace w;
        w.grid = c.take<KnnGrid>(1); w.cell_of = c.take<uint32_t>(P); w.cell_count = c.take<uint32_t>(C); w.cell_start = c.take<uint32_t>(C + 1);
        w.cursor = c.take<uint32_t>(C); w.sorted_pts = c.take<float4>(P);
        w.bytes = c.bytes();
        return w;
    }
};
static inline size_t knn_max_cells(int P) { return (size_t)(P < 64 ? 64 : P); }

size_t gsr_knn_workspace_size(int P) { return KnnWorkspace::from(nullptr, (size_t)(P > 0 ? P : 1), knn_max_cells(P)).bytes; }

int gsr_knn_mean_dist2(int P, const float* points, float* mean_dists, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (P > 0 && (!points || !mean_dists || !workspace))) { g_last_error = "gsr_knn_mean_dist2: null argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P == 0) return 0;
    const size_t C = knn_max_cells(P);
    const KnnWorkspace w = KnnWorkspace::from(workspace, (size_t)P, C);
    ScopedKernelTimer tm(K_KNN, stream);
    GSR_HIP_CHECK(hipMemsetAsync(w.grid, 0xFF, 3 * sizeof(uint32_t), stream));                       // bbox min = ~0
    GSR_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char*>(w.grid) + 12, 0x00, 3 * sizeof(uint32_t), stream));   // bbox max = 0
    GSR_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, C * sizeof(uint32_t), stream));
    const int nb = (P + 255) / 256;
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, stream, P, points, w.grid);
    hipLaunchKernelGGL(knn_setup_kernel, dim3(1), dim3(1), 0, stream, P, (int)C, w.grid);
    hipLaunchKernelGGL(knn_count_kernel, dim3(nb), dim3(256), 0, stream, P, points, w.grid, w.cell_of, w.cell_count);
    hipLaunchKernelGGL(knn_scan_kernel, dim3(1), dim3(1024), 0, stream, w.grid, w.cell_count, w.cell_start, w.cursor);
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(nb), dim3(256), 0, stream, P, points, w.cell_of, w.cursor, w.sorted_pts);
    hipLaunchKernelGGL(knn_query_kernel, dim3(nb), dim3(256), 0, stream, P, w.grid, w.cell_start, w.sorted_pts, mean_dists);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}


// Test hook: runs gsr::wave_sum10_transposed on one wave. in: device float[64][10]; out: device float[64] (what each lane holds).
__global__ void debug_reduce10_kernel(const float* in, float* out)
{
    const int l = threadIdx.x;
    const float* v = in + l * 10;
    unsigned long long proc = 0; uint32_t addr;
    out[l] = wave_sum10_transposed(wave_select_masks(), v[0], f2v{v[1], v[2]}, f2v{v[3], v[4]}, v[5], f2v{v[6], v[7]}, f2v{v[8], v[9]}, proc, 0, 0u, 0, addr);
}
// the work-item map of gs_device.h on the host (no device needed): block index of the full piece of rank `rank` (partial = 0) or of the
// partial piece of rank `rank` (partial = 1) in a frame of n_items pieces, n_partial of them partial
int gsr_debug_item_block(unsigned int n_items, unsigned int n_partial, unsigned int rank, int partial)
{
    if (n_partial > n_items || rank >= (partial ? n_partial : n_items - n_partial)) return GSR_ERR_INVALID_ARGUMENT;
    return (int)(partial ? item_block_partial(n_items, n_partial, rank) : item_block_full(n_items, n_partial, rank));
}
int gsr_debug_wave_reduce10(const float* in, float* out, void* stream_)
{
    hipLaunchKernelGGL(debug_reduce10_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, in, out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}


// ---- fused L1 loss (include/slam_losses.h) ------------------------------------------------------------------------
size_t gsr_l1_loss_workspace_size(void) { return (size_t)LOSS_BLOCKS * 2 * sizeof(float); }

static LossArgs make_loss_args(int width, int height, const float* image, const float* depth, const float* gt_image, const float* gt_depth,
                               const float* w_rgb, const float* w_depth, const float* exposure_a, const float* exposure_b, float alpha,
                               const float* opacity, float opacity_thr)
{
    LossArgs a;
    a.opacity = opacity; a.opacity_thr = opacity_thr;
    a.N = width * height; a.image = image; a.depth = depth; a.gt_image = gt_image; a.gt_depth = gt_depth; a.w_rgb = w_rgb; a.w_depth = w_depth;
    a.exposure_a = exposure_a; a.exposure_b = exposure_b;
    a.c_rgb = alpha / (3.0f * (float)a.N); a.c_depth = (1.0f - alpha) / (float)a.N;
    return a;
}

int gsr_l1_loss_forward(int width, int height, const float* image, const float* depth, const float* gt_image, const float* gt_depth,
                        const float* w_rgb, const float* w_depth, const float* exposure_a, const float* exposure_b, float alpha,
                        const float* opacity, float opacity_depth_threshold, float* loss, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (width <= 0 || height <= 0 || !image || !depth || !gt_image || !gt_depth || !loss || !workspace) {
        g_last_error = "gsr_l1_loss_forward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const LossArgs a = make_loss_args(width, height, image, depth, gt_image, gt_depth, w_rgb, w_depth, exposure_a, exposure_b, alpha, opacity,
                                      opacity_depth_threshold);
    float* partials = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(l1_loss_fwd_kernel, dim3(LOSS_BLOCKS), dim3(LOSS_THREADS), 0, stream, a, partials);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, stream, (const float*)partials, 1, loss);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_l1_loss_backward(int width, int height, const float* image, const float* depth, const float* gt_image, const float* gt_depth,
                         const float* w_rgb, const float* w_depth, const float* exposure_a, const float* exposure_b, float alpha,
                         const float* opacity, float opacity_depth_threshold, const float* upstream, float* dL_dimage, float* dL_ddepth, float* dL_dexposure, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (width <= 0 || height <= 0 || !image || !depth || !gt_image || !gt_depth || !dL_dimage || !dL_ddepth || !workspace) {
        g_last_error = "gsr_l1_loss_backward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const LossArgs a = make_loss_args(width, height, image, depth, gt_image, gt_depth, w_rgb, w_depth, exposure_a, exposure_b, alpha, opacity,
                                      opacity_depth_threshold);
    float* partials = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(l1_loss_bwd_kernel, dim3(LOSS_BLOCKS), dim3(LOSS_THREADS), 0, stream, a, upstream, dL_dimage, dL_ddepth, partials);
    if (dL_dexposure) hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, stream, (const float*)partials, 2, dL_dexposure);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}


static int masked_l1_args(MaskedL1Args& a, int n_terms, const gsr_masked_l1_term* terms, int width, int height, int channels, int image_channels,
                          float scale, bool backward, const char* who)
{
    static thread_local std::string msg;
    bool ok = n_terms >= 1 && n_terms <= MASKED_L1_MAX_TERMS && terms && width > 0 && height > 0 && channels >= 1 && channels <= image_channels;
    for (int t = 0; ok && t < n_terms; t++) ok = terms[t].image && terms[t].target && terms[t].mask && (!backward || terms[t].dL_dimage);
    if (!ok) { msg = std::string(who) + ": null / invalid argument (1 <= n_terms <= 4, 1 <= channels <= image_channels)"; g_last_error = msg.c_str(); return GSR_ERR_INVALID_ARGUMENT; }
    a = MaskedL1Args{};
    a.n_terms = n_terms; a.N = width * height; a.C = channels; a.Cimg = image_channels;
    for (int t = 0; t < n_terms; t++) { a.image[t] = terms[t].image; a.target[t] = terms[t].target; a.mask[t] = terms[t].mask; a.dL_dimage[t] = terms[t].dL_dimage; }
    a.coeff = scale / ((float)channels * (float)a.N);
    return 0;
}

int gsr_masked_l1_forward(int n_terms, const gsr_masked_l1_term* terms, int width, int height, int channels, int image_channels, float scale,
                          float* loss, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    MaskedL1Args a;
    const int rc = masked_l1_args(a, n_terms, terms, width, height, channels, image_channels, scale, false, "gsr_masked_l1_forward");
    if (rc < 0) return rc;
    if (!loss || !workspace) { g_last_error = "gsr_masked_l1_forward: null loss / workspace"; return GSR_ERR_INVALID_ARGUMENT; }
    float* partials = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(masked_l1_fwd_kernel, dim3(LOSS_BLOCKS), dim3(LOSS_THREADS), 0, stream, a, partials);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, stream, (const float*)partials, 1, loss);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_masked_l1_backward(int n_terms, const gsr_masked_l1_term* terms, int width, int height, int channels, int image_channels, float scale,
                           const float* upstream, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    MaskedL1Args a;
    const int rc = masked_l1_args(a, n_terms, terms, width, height, channels, image_channels, scale, true, "gsr_masked_l1_backward");
    if (rc < 0) return rc;
    hipLaunchKernelGGL(masked_l1_bwd_kernel, dim3(LOSS_BLOCKS, (unsigned)n_terms), dim3(LOSS_THREADS), 0, stream, a, upstream);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- fused Adam (include/slam_losses.h) ---------------------------------------------------------------------------
void gsr_adam_coefficients(double lr, double beta1, double beta2, int step, float out[2])
{
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    out[0] = (float)(lr / bc1); out[1] = (float)(1.0 / sqrt(bc2));
}

static int adam_step_impl(int nseg, const gsr_adam_segment* segs, const float* coefficients, bool scheduled, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (nseg < 0 || nseg > ADAM_MAX_SEGMENTS || (nseg > 0 && !segs)) { g_last_error = "gsr_adam_step: 0..32 segments"; return GSR_ERR_INVALID_ARGUMENT; }
    if (scheduled && nseg > 0 && !coefficients) { g_last_error = "gsr_adam_step_scheduled: null coefficients"; return GSR_ERR_INVALID_ARGUMENT; }
    AdamArgs a;
    a.nseg = nseg; a.total = 0; a.coef = scheduled ? coefficients : nullptr;
    for (int k = 0; k < nseg; k++) {
        const gsr_adam_segment& h = segs[k];
        if (h.n && (!h.param || !h.grad || !h.exp_avg || !h.exp_avg_sq)) { g_last_error = "gsr_adam_step: null pointer"; return GSR_ERR_INVALID_ARGUMENT; }
        if (!scheduled && h.step < 1) { g_last_error = "gsr_adam_step: step counts from 1"; return GSR_ERR_INVALID_ARGUMENT; }
        a.start[k] = a.total;
        AdamSegment& d = a.seg[k];
        d.param = h.param; d.grad = h.grad; d.exp_avg = h.exp_avg; d.exp_avg_sq = h.exp_avg_sq; d.n = h.n;
        float c[2] = {0.f, 0.f};
        if (!scheduled) gsr_adam_coefficients((double)h.lr, h.beta1_d, h.beta2_d, h.step, c);
        d.step_size = c[0]; d.inv_bc2_sqrt = c[1]; d.eps = h.eps; d.beta2 = h.beta2;
        d.one_minus_beta1 = (float)(1.0 - h.beta1_d); d.one_minus_beta2 = (float)(1.0 - h.beta2_d);
        a.total += h.n;
    }
    a.start[nseg] = a.total;
    if (a.total == 0) return 0;
    const unsigned long long blocks = (a.total + 255) / 256;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}
int gsr_adam_step(int nseg, const gsr_adam_segment* segs, void* stream) { return adam_step_impl(nseg, segs, nullptr, false, stream); }
int gsr_adam_step_device_count(int nseg, const gsr_adam_segment* segs, float* const* step_counts, float* coefficients, void* stream_)
{
    if (nseg < 0 || nseg > ADAM_MAX_SEGMENTS || (nseg > 0 && (!segs || !step_counts || !coefficients))) {
        g_last_error = "gsr_adam_step_device_count: 0..32 segments, no null arguments"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (nseg == 0) return 0;
    AdamDeviceSteps d;
    d.nseg = nseg;
    for (int k = 0; k < nseg; k++) {
        if (!step_counts[k]) { g_last_error = "gsr_adam_step_device_count: null step count"; return GSR_ERR_INVALID_ARGUMENT; }
        d.step[k] = step_counts[k]; d.lr[k] = segs[k].lr; d.beta1[k] = segs[k].beta1_d; d.beta2[k] = segs[k].beta2_d;
    }
    hipLaunchKernelGGL(adam_device_coefficients_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, d, coefficients);
    GSR_HIP_CHECK(hipGetLastError());
    return adam_step_impl(nseg, segs, coefficients, true, stream_);
}
int gsr_adam_step_scheduled(int nseg, const gsr_adam_segment* segs, const float* coefficients, void* stream)
{
    return adam_step_impl(nseg, segs, coefficients, true, stream);
}


// ---- fused SSIM (include/slam_losses.h) ---------------------------------------------------------------------------
static SsimWindow ssim_window()
{
    SsimWindow w;                                          // loss_utils.py:46-53: exp(-(x - 5)^2 / (2 * 1.5^2)), normalised
    double sum = 0.0, g[SSIM_WIN];
    for (int k = 0; k < SSIM_WIN; k++) { g[k] = exp(-(double)((k - SSIM_R) * (k - SSIM_R)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < SSIM_WIN; k++) w.w[k] = (float)((float)g[k] / (float)sum);
    return w;
}
static inline dim3 ssim_grid(int width, int height, int channels)
{
    return dim3((width + SSIM_T - 1) / SSIM_T, (height + SSIM_T - 1) / SSIM_T, channels);
}
// workspace of the SSIM pair: one partial sum per block of the forward launch | the three derivative maps [3, C, H, W] the backward pass reads
struct SsimWs { int nblocks; float* partials; float* dmaps; size_t bytes; };
static SsimWs ssim_layout(int width, int height, int channels, const char* workspace)
{
    const bool ok = width > 0 && height > 0 && channels > 0;
    const dim3 g = ssim_grid(width, height, channels);
    const int nblocks = ok ? (int)(g.x * g.y * g.z) : 0;
    Carver c(workspace, 256);
    return {nblocks, c.take<float>((size_t)nblocks), c.take<float>(ok ? (size_t)3 * channels * width * height : 0), c.bytes()};
}
size_t gsr_ssim_workspace_size(int width, int height, int channels) { return ssim_layout(width, height, channels, nullptr).bytes; }

int gsr_ssim_forward(int width, int height, int channels, const float* img1, const float* img2, const unsigned char* mask, float* ssim_mean,
                     char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (width <= 0 || height <= 0 || channels <= 0 || !img1 || !img2 || !ssim_mean || !workspace) {
        g_last_error = "gsr_ssim_forward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const dim3 g = ssim_grid(width, height, channels);
    const SsimWs w = ssim_layout(width, height, channels, workspace);
    hipLaunchKernelGGL(ssim_fwd_kernel, g, dim3(SSIM_T * SSIM_T), 0, stream, width, height, img1, img2, mask, ssim_window(), w.dmaps, w.partials);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, stream, w.nblocks, (const float*)w.partials,
                       1.0f / ((float)channels * (float)width * (float)height), ssim_mean);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_ssim_backward(int width, int height, int channels, const float* img1, const float* img2, const unsigned char* mask,
                      const float* upstream, float* dL_dimg1, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (width <= 0 || height <= 0 || channels <= 0 || !img1 || !img2 || !dL_dimg1 || !workspace) {
        g_last_error = "gsr_ssim_backward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const dim3 g = ssim_grid(width, height, channels);
    const float* dmaps = ssim_layout(width, height, channels, workspace).dmaps;
    hipLaunchKernelGGL(ssim_bwd_kernel, g, dim3(SSIM_T * SSIM_T), 0, stream, width, height, img1, img2, mask, ssim_window(), dmaps, upstream,
                       1.0f / ((float)channels * (float)width * (float)height), dL_dimg1);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}


int gsr_densification_stats(int P, const int* radii, const float* grad_mean2D, float* max_radii2D, float* xyz_gradient_accum, float* denom,
                            void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || (P > 0 && (!radii || !grad_mean2D || !max_radii2D || !xyz_gradient_accum || !denom))) {
        g_last_error = "gsr_densification_stats: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return 0;
    hipLaunchKernelGGL(densification_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, radii, grad_mean2D, max_radii2D,
                       xyz_gradient_accum, denom);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}


int gsr_hexplane_forward(const gsr_hexplane_field* field, int64_t n, const float* xyz, int64_t xyz_stride, const float* time,
                         int64_t time_stride, float* features, void* stream_)
{
    if (int rc = hexplane_check(field, n, xyz, time, "gsr_hexplane_forward")) return rc;
    if (n == 0) return 0;
    if (!features) { g_last_error = "gsr_hexplane_forward: null features"; return GSR_ERR_INVALID_ARGUMENT; }
    hexplane_launch<false>(*field, n, (hipStream_t)stream_, xyz, xyz_stride, time, time_stride, features);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static void hexsort_plan(const gsr_hexplane_field& f, HexSortPlan* P)
{
    for (int k = 0; k < 4; k++) {
        int r = 1;
        for (int l = 0; l < f.num_levels; l++) r = std::max(r, (int)f.levels[l].res[k]);
        P->fine[k] = r;
        int b = 0;
        while ((1 << b) < r) b++;
        P->bits[k] = b;
    }
    int off = 0;
    for (int pl = 0; pl < 6; pl++) {
        // every call of the reference passes ONE time for all points (gaussian_renderer/__init__.py:112): the time families then use a
        // single row of cells, n / 512 points per cell -- give them 16 sub-counters per cell (the spatial families: 2), up to 2^20 counters
        const int cell_bits = P->bits[hex_c0(pl)] + P->bits[hex_c1(pl)];
        P->sub_bits[pl] = std::max(0, std::min(hex_c1(pl) == 3 ? 4 : 1, 20 - cell_bits));
        P->key_off[pl] = off;
        off += 1 << (cell_bits + P->sub_bits[pl]);
    }
    P->key_off[6] = off;
}

// ---- the workspace of the sorted backward passes -------------------------------------------------------------------------------
// What one sorted backward call keeps in its workspace: the sort's regions, the route's own staging of dL/dsample (ws.gs, or vw), the ordered sums.
struct HexBwdWs {
    HexSortPlan P;
    HexSortWs ws;
    HexViewsWs vw;          // batched views only
    HexOrd ord;             // acc null: float atomics
    size_t ord_bytes;       // of acc and acc_t, one region (one memset)
    size_t total;           // of the whole workspace
};

// The planes the generic walk scatters into: all six, or the three spatial ones of the batched views (their time families keep column sums per view)
constexpr int HEX_ALL_PLANES = 63, HEX_SPATIAL_PLANES = (1 << 0) | (1 << 1) | (1 << 3);

static void hexsort_carve_head(Carver& c, const gsr_hexplane_field& f, int64_t n, HexBwdWs* L)
{
    hexsort_plan(f, &L->P);
    const size_t nb = (size_t)L->P.key_off[6];
    HexSortWs& w = L->ws;
    w.count = c.take<uint32_t>(nb);
    w.block_sums = c.take<uint32_t>(nb / (1024 * HEXSORT_SCAN_ITEMS) + 1);
    w.header = c.take<uint32_t>(64);
    w.coords = c.take<float4>((size_t)n);
    w.key = c.take<uint32_t>((size_t)6 * n);
    w.rank = c.take<int>((size_t)6 * n);
    w.scoords = c.take<float4>((size_t)6 * n);
}

// Ordered mode (HexOrd): where the fixed-point sums of the planes in `plane_mask` live and, for the V > 0 views of the batched path, the time
// families' column sums. Closes the carve.
static void hexord_carve_tail(Carver& c, const gsr_hexplane_field& f, int64_t n, int V, int plane_mask, bool ordered, HexBwdWs* L)
{
    if (ordered) {
        HexOrd& h = L->ord;
        size_t elems = 0, rows = 0;
        for (int l = 0; l < f.num_levels; l++)
            for (int pl = 0; pl < 6; pl++) {
                h.off[l][pl] = elems;
                if ((plane_mask >> pl) & 1) elems +=    // (whether or not the plane's gradient is asked for: the size must not depend on it)
                    (size_t)f.levels[l].res[hex_c0(pl)] * f.levels[l].res[hex_c1(pl)] * f.feat_dim;
            }
        if (V > 0)
            for (int j = 0; j < 3; j++) {
                uint32_t cols = 0;
                for (int l = 0; l < f.num_levels; l++) { h.tcol[j][l] = cols; cols += (uint32_t)f.levels[l].res[j]; }
                h.tcols[j] = cols;
                h.tbase[j] = (uint32_t)rows;
                rows += (size_t)V * cols;
            }
        // a texel receives at most 4 n contributions (four cells, every point once: the views are summed before): the largest one is scaled to just
        // below 2^budget, the sum stays below 2^62; 40 bits at most, so that HEXSORT_CHUNK of them stay exact in a double
        int lg = 0;
        while (((int64_t)1 << lg) < 4 * std::max<int64_t>(n, 1)) lg++;
        h.budget = std::min(40, 62 - lg);
        const size_t all = elems + rows * f.feat_dim;
        h.acc = c.take<unsigned long long>(all);
        if (V > 0 && h.acc) h.acc_t = h.acc + elems;
        L->ord_bytes = all * sizeof(unsigned long long);
    }
    L->total = c.bytes_padded();
}

static HexBwdWs hexsort_carve(const gsr_hexplane_field& f, int64_t n, bool ordered, char* base)
{
    HexBwdWs L{};
    Carver c(base, 256, true);
    hexsort_carve_head(c, f, n, &L);
    L.ws.gs = c.take<float>((size_t)6 * n * f.num_levels * f.feat_dim);
    hexord_carve_tail(c, f, n, 0, HEX_ALL_PLANES, ordered, &L);
    return L;
}

static int hexsort_check_workspace(const char* who, const HexBwdWs& L, size_t workspace_bytes)
{
    if (workspace_bytes >= L.total) return 0;
    g_last_error = std::string(who) + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(L.total) +
                   " needed (was \"hex_ordered\" set after the size query?)";
    return GSR_ERR_INVALID_ARGUMENT;
}

// How both sorted passes begin: clear the counters (ordered mode: the header's maximum and the sums too), count, scan, move the points into
// sorted order. The single-time pass gives time and dL_dfeatures, the batched one its view_mask.
static int hexsort_prologue(const gsr_hexplane_field& f, const HexBwdWs& L, int64_t n, const float* xyz, int64_t xyz_stride, const float* time,
                            int64_t time_stride, const float* dL_dfeatures, const uint32_t* view_mask, hipStream_t stream)
{
    const HexSortWs& ws = L.ws;
    const int nb = L.P.key_off[6], scan_blocks = (nb + 1024 * HEXSORT_SCAN_ITEMS - 1) / (1024 * HEXSORT_SCAN_ITEMS);
    GSR_HIP_CHECK(hipMemsetAsync(ws.count, 0, (size_t)nb * sizeof(uint32_t), stream));
    if (L.ord.acc) {
        GSR_HIP_CHECK(hipMemsetAsync(ws.header, 0, 256, stream));
        GSR_HIP_CHECK(hipMemsetAsync(L.ord.acc, 0, L.ord_bytes, stream));
    }
    hipLaunchKernelGGL(hexsort_count_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, stream, f, L.P, ws, n, xyz, xyz_stride, time, time_stride,
                       dL_dfeatures, view_mask);
    hipLaunchKernelGGL(hexsort_scan_sums_kernel, dim3(scan_blocks), dim3(1024), 0, stream, (const uint32_t*)ws.count, nb, ws.block_sums);
    hipLaunchKernelGGL(hexsort_scan_top_kernel, dim3(1), dim3(1024), 0, stream, ws.block_sums, scan_blocks, ws.header);
    hipLaunchKernelGGL(hexsort_scan_apply_kernel, dim3(scan_blocks), dim3(1024), 0, stream, ws.count, nb, (const uint32_t*)ws.block_sums);
    hipLaunchKernelGGL(hexsort_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, n);
    return 0;
}

static void hexord_convert(const gsr_hexplane_field& f, const HexOrd& ord, const uint32_t* header, int plane_mask, hipStream_t stream)
{
    size_t largest = 0;
    for (int l = 0; l < f.num_levels; l++)
        for (int pl = 0; pl < 6; pl++)
            largest = std::max(largest, (size_t)f.levels[l].res[hex_c0(pl)] * f.levels[l].res[hex_c1(pl)] * f.feat_dim);
    hipLaunchKernelGGL(hexord_convert_kernel, dim3((unsigned)((largest + 511) / 512), (unsigned)(6 * f.num_levels)), dim3(256), 0, stream, f, ord, header,
                       plane_mask);
}

static bool hexsort_supported(const gsr_hexplane_field& f, int64_t n)
{
    if (!f.channels_last || n * 6 >= ((int64_t)1 << 31)) return false;
    for (int l = 0; l < f.num_levels; l++)
        for (int k = 0; k < 4; k++) if (f.levels[l].res[k] > 1024) return false;   // 2 x 10 key bits per family
    return true;
}

size_t gsr_hexplane_backward_workspace_size(const gsr_hexplane_field* field, int64_t n)
{
    if (!field || n <= 0 || field->num_levels < 1 || field->num_levels > GSR_HEXPLANE_MAX_LEVELS || !hexsort_supported(*field, n)) return 256;
    return hexsort_carve(*field, n, g_hex_ordered.load() != 0, nullptr).total;
}

int gsr_hexplane_backward(const gsr_hexplane_field* field, int64_t n, const float* xyz, int64_t xyz_stride, const float* time,
                          int64_t time_stride, const float* dL_dfeatures, float* dL_dxyz, char* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = hexplane_check(field, n, xyz, time, "gsr_hexplane_backward")) return rc;
    if (n == 0) return 0;
    if (!dL_dfeatures) { g_last_error = "gsr_hexplane_backward: null dL_dfeatures"; return GSR_ERR_INVALID_ARGUMENT; }
    const gsr_hexplane_field& f = *field;
    if (!workspace || !hexsort_supported(f, n)) {
        hexplane_launch<true>(f, n, stream, xyz, xyz_stride, time, time_stride, dL_dfeatures, dL_dxyz);
        GSR_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const HexBwdWs L = hexsort_carve(f, n, g_hex_ordered.load() != 0, workspace);      // the mode of this call, read once
    if (int rc = hexsort_check_workspace("gsr_hexplane_backward", L, workspace_bytes)) return rc;
    if (int rc = hexsort_prologue(f, L, n, xyz, xyz_stride, time, time_stride, dL_dfeatures, nullptr, stream)) return rc;
    const HexSortWs& ws = L.ws;
    const HexOrd& ord = L.ord;
    const int ordered = ord.acc != nullptr;
    const int C = f.feat_dim, ppb = HEX_BLOCK / C;
    const dim3 g1((unsigned)((n + ppb - 1) / ppb));
    const int64_t groups = 6 * ((n + HEXSORT_CHUNK - 1) / HEXSORT_CHUNK);
    const dim3 g2((unsigned)((groups + 256 / C - 1) / (256 / C)));
#define GSR_HEXSORT_CASE(CC)                                                                                                              \
    case CC:                                                                                                                               \
        hipLaunchKernelGGL((hexsort_phase1_kernel<CC>), g1, dim3(HEX_BLOCK), 0, stream, f, ws, n, xyz, xyz_stride, time, time_stride,       \
                           dL_dfeatures, dL_dxyz, ordered);                                                                                 \
        if (f.num_levels <= 4) {                                                                                                           \
            if (ordered) hipLaunchKernelGGL((hexsort_phase2_kernel<CC, 4, true>), g2, dim3(256), 0, stream, f, ws, n, ord);                 \
            else hipLaunchKernelGGL((hexsort_phase2_kernel<CC, 4, false>), g2, dim3(256), 0, stream, f, ws, n, ord);                        \
        } else {                                                                                                                           \
            if (ordered) hipLaunchKernelGGL((hexsort_phase2_kernel<CC, GSR_HEXPLANE_MAX_LEVELS, true>), g2, dim3(256), 0, stream, f, ws, n, ord);   \
            else hipLaunchKernelGGL((hexsort_phase2_kernel<CC, GSR_HEXPLANE_MAX_LEVELS, false>), g2, dim3(256), 0, stream, f, ws, n, ord);          \
        }                                                                                                                                  \
        break;
    switch (C) { GSR_HEXSORT_CASE(8) GSR_HEXSORT_CASE(16) GSR_HEXSORT_CASE(32) GSR_HEXSORT_CASE(64) }
#undef GSR_HEXSORT_CASE
    if (ordered) hexord_convert(f, ord, ws.header, HEX_ALL_PLANES, stream);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the views of one mapping iteration (include/deformation_field.h) ----------------------------------------------------------------
static int hexplane_views_check(const gsr_hexplane_field* f, int64_t n, const float* xyz, int V, const float* times, const char* who)
{
    static const float some_time = 0.f;
    if (int rc = hexplane_check(f, n, xyz, &some_time, who)) return rc;
    if (V < 1 || V > GSR_HEXPLANE_MAX_VIEWS || !times) {
        g_last_error = std::string(who) + ": 1 <= V <= GSR_HEXPLANE_MAX_VIEWS times (host pointer) expected";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return 0;
}
static HexTimes hex_times(int V, const float* times)
{
    HexTimes tv{};
    tv.V = V;
    for (int v = 0; v < V; v++) tv.t[v] = times[v];
    return tv;
}

int gsr_hexplane_forward_views(const gsr_hexplane_field* field, int64_t n, const float* xyz, int64_t xyz_stride, int V, const float* times,
                               float* features, void* stream_)
{
    if (int rc = hexplane_views_check(field, n, xyz, V, times, "gsr_hexplane_forward_views")) return rc;
    if (n == 0) return 0;
    if (!features) { g_last_error = "gsr_hexplane_forward_views: null features"; return GSR_ERR_INVALID_ARGUMENT; }
    const gsr_hexplane_field& f = *field;
    const HexTimes tv = hex_times(V, times);
    const int lpp = f.feat_dim / 4;
    const dim3 grid((unsigned)((n + HEX_BLOCK / lpp - 1) / (HEX_BLOCK / lpp))), block(HEX_BLOCK);
    hipStream_t stream = (hipStream_t)stream_;
#define GSR_HEXV_CASE(LPP)                                                                                                              \
    case LPP:                                                                                                                           \
        if (f.channels_last) hipLaunchKernelGGL((hexplane_fwd_views_kernel<LPP, HEX_VEC>), grid, block, 0, stream, f, n, xyz, xyz_stride, tv, features);   \
        else hipLaunchKernelGGL((hexplane_fwd_views_kernel<LPP, HEX_PLANAR>), grid, block, 0, stream, f, n, xyz, xyz_stride, tv, features);               \
        break;
    switch (lpp) { GSR_HEXV_CASE(2) GSR_HEXV_CASE(4) GSR_HEXV_CASE(8) GSR_HEXV_CASE(16) }
#undef GSR_HEXV_CASE
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static HexBwdWs hexviews_carve(const gsr_hexplane_field& f, int64_t n, int V, bool ordered, char* base)
{
    HexBwdWs L{};
    Carver c(base, 256, true);
    hexsort_carve_head(c, f, n, &L);
    const size_t row = (size_t)f.num_levels * f.feat_dim;
    L.vw.gs_sp = c.take<float>((size_t)3 * n * row);
    L.vw.gs_t = c.take<float>((size_t)3 * V * n * row);
    hexord_carve_tail(c, f, n, V, HEX_SPATIAL_PLANES, ordered, &L);
    return L;
}

static bool hexviews_supported(const gsr_hexplane_field& f, int64_t n)
{
    // (the time families' LDS window is [4 views][4 or 8 levels][16 columns][C] floats: 64 channels with more than four levels would be 128 KB)
    return hexsort_supported(f, n) && !(f.feat_dim == 64 && f.num_levels > 4);
}

size_t gsr_hexplane_backward_views_workspace_size(const gsr_hexplane_field* field, int64_t n, int V)
{
    if (!field || n <= 0 || V < 1 || V > GSR_HEXPLANE_MAX_VIEWS || field->num_levels < 1 || field->num_levels > GSR_HEXPLANE_MAX_LEVELS ||
        !hexviews_supported(*field, n)) return 0;
    return hexviews_carve(*field, n, V, g_hex_ordered.load() != 0, nullptr).total;
}

int gsr_hexplane_backward_views(const gsr_hexplane_field* field, int64_t n, const float* xyz, int64_t xyz_stride, int V, const float* times,
                                const float* dL_dfeatures, const uint32_t* view_mask, float* dL_dxyz, char* workspace, size_t workspace_bytes,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = hexplane_views_check(field, n, xyz, V, times, "gsr_hexplane_backward_views")) return rc;
    if (n == 0) return 0;
    const gsr_hexplane_field& f = *field;
    if (!dL_dfeatures || !workspace || !hexviews_supported(f, n)) {
        g_last_error = "gsr_hexplane_backward_views: null cotangent / workspace, or a geometry the sorted algorithm does not cover (see gsr_hexplane_backward_views_workspace_size)";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const HexTimes tv = hex_times(V, times);
    const HexBwdWs L = hexviews_carve(f, n, V, g_hex_ordered.load() != 0, workspace);  // the mode of this call, read once
    if (int rc = hexsort_check_workspace("gsr_hexplane_backward_views", L, workspace_bytes)) return rc;
    if (int rc = hexsort_prologue(f, L, n, xyz, xyz_stride, nullptr, 0, nullptr, view_mask, stream)) return rc;
    const HexSortWs& ws = L.ws;
    const HexViewsWs& vw = L.vw;
    const HexOrd& ord = L.ord;
    const int ordered = ord.acc != nullptr;
    const int C = f.feat_dim, ppb = HEX_BLOCK / C;
    const dim3 g1((unsigned)((n + ppb - 1) / ppb));
    const int gpw = C >= 64 ? 1 : 64 / C;                        // groups per wave (hexsort_phase2_views_kernel)
    const int64_t chunks2 = (n + HEXSORT_CHUNK - 1) / HEXSORT_CHUNK;
    const int64_t groups = (int64_t)3 * ((chunks2 + gpw - 1) / gpw) * gpw;
    const dim3 g2((unsigned)((groups + 256 / C - 1) / (256 / C)));
    const int per_block = (256 / C) * HEXT_ROUNDS;               // chunks per block of the time families' kernel
    const dim3 g3((unsigned)((chunks2 + per_block - 1) / per_block), (unsigned)(3 * ((V + HEXT_VB - 1) / HEXT_VB)));
#define GSR_HEXVB_CASE(CC)                                                                                                              \
    case CC:                                                                                                                             \
        hipLaunchKernelGGL((hexsort_phase1_views_kernel<CC>), g1, dim3(HEX_BLOCK), 0, stream, f, ws, vw, tv, n, xyz, xyz_stride, dL_dfeatures, dL_dxyz, ordered);   \
        GSR_HEXVB_PHASE2(CC, 4, f.num_levels <= 4)                                                                                       \
        GSR_HEXVB_PHASE2(CC, GSR_HEXPLANE_MAX_LEVELS, f.num_levels > 4)                                                                  \
        break;
#define GSR_HEXVB_PHASE2(CC, LM, when)                                                                                                  \
        if (when) {                                                                                                                     \
            if (ordered) {                                                                                                              \
                hipLaunchKernelGGL((hexsort_phase2_views_kernel<CC, LM, true>), g2, dim3(256), 0, stream, f, ws, vw, n, ord);                        \
                hipLaunchKernelGGL((hexsort_phase2_time_kernel<CC, LM, true>), g3, dim3(256), 0, stream, f, ws, vw, tv, n, ord);                     \
            } else {                                                                                                                    \
                hipLaunchKernelGGL((hexsort_phase2_views_kernel<CC, LM, false>), g2, dim3(256), 0, stream, f, ws, vw, n, ord);                       \
                hipLaunchKernelGGL((hexsort_phase2_time_kernel<CC, LM, false>), g3, dim3(256), 0, stream, f, ws, vw, tv, n, ord);                    \
            }                                                                                                                           \
        }
    switch (C) { GSR_HEXVB_CASE(8) GSR_HEXVB_CASE(16) GSR_HEXVB_CASE(32) GSR_HEXVB_CASE(64) }
#undef GSR_HEXVB_PHASE2
#undef GSR_HEXVB_CASE
    if (ordered) {
        hexord_convert(f, ord, ws.header, HEX_SPATIAL_PLANES, stream);
        int wmax = 1;
        for (int l = 0; l < f.num_levels; l++)
            for (int k = 0; k < 3; k++) wmax = std::max(wmax, (int)f.levels[l].res[k]);
        hipLaunchKernelGGL(hexord_time_convert_kernel, dim3((unsigned)(((size_t)wmax * C + 255) / 256), (unsigned)(3 * f.num_levels)), dim3(256), 0, stream, f, tv,
                           ord, (const uint32_t*)ws.header);
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- dense-layer weight gradient (include/deformation_field.h) -----------------------------------------------------------------
static void wgrad_plan(int64_t n, int64_t* chunk, int* nblocks)
{
    int64_t c = (n + 511) / 512;                                  // ~512 blocks along the reduction (2 per CU)
    c = ((c + 4 * WGRAD_UNROLL - 1) / (4 * WGRAD_UNROLL)) * (4 * WGRAD_UNROLL);
    if (c < 64) c = 64;
    *chunk = c;
    *nblocks = (int)((n + c - 1) / c);
}

size_t gsr_linear_wgrad_workspace_size(int64_t n, int in_dim, int out_dim)
{
    if (n <= 0 || in_dim <= 0 || out_dim <= 0) return 256;
    int64_t chunk; int nb;
    wgrad_plan(n, &chunk, &nb);
    return (size_t)nb * out_dim * (in_dim + 1) * sizeof(float) + 256;
}

int gsr_linear_wgrad(int64_t n, int in_dim, int out_dim, const float* x, int64_t x_stride, const float* dy, int64_t dy_stride,
                     float* dW, float* db, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || in_dim <= 0 || in_dim > 128 || out_dim <= 0 || (n > 0 && (!x || !dy || !workspace)) || (!dW && !db)) {
        g_last_error = "gsr_linear_wgrad: null / invalid argument (in_dim must be 1..128)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) {
        if (dW) GSR_HIP_CHECK(hipMemsetAsync(dW, 0, (size_t)out_dim * in_dim * sizeof(float), stream));
        if (db) GSR_HIP_CHECK(hipMemsetAsync(db, 0, (size_t)out_dim * sizeof(float), stream));
        return 0;
    }
    int64_t chunk; int nb;
    wgrad_plan(n, &chunk, &nb);
    float* partial = reinterpret_cast<float*>(workspace);
    const dim3 grid((unsigned)nb, (unsigned)((out_dim + 63) / 64)), block(WGRAD_BLOCK);
    const int nt = (in_dim + 15) / 16;
    switch (nt) {
#define GSR_WGRAD_CASE(NT) case NT: hipLaunchKernelGGL((linear_wgrad_kernel<NT>), grid, block, 0, stream, n, in_dim, out_dim, x, x_stride, dy, dy_stride, partial, chunk); break;
        GSR_WGRAD_CASE(1) GSR_WGRAD_CASE(2) GSR_WGRAD_CASE(3) GSR_WGRAD_CASE(4) GSR_WGRAD_CASE(5) GSR_WGRAD_CASE(6) GSR_WGRAD_CASE(7) GSR_WGRAD_CASE(8)
#undef GSR_WGRAD_CASE
    }
    const int per = out_dim * (in_dim + 1);
    hipLaunchKernelGGL(linear_wgrad_reduce_kernel, dim3((per + WRED_OUT - 1) / WRED_OUT), dim3(WRED_OUT * WRED_SLICES), 0, stream, nb, in_dim, out_dim,
                       (const float*)partial, dW, db);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- fused deformation MLP (include/deformation_field.h) ------------------------------------------------------------------------------
static int mlp_fill(const gsr_deform_mlp* m, MlpWeights* w, const char* who)
{
    static thread_local std::string msg;
    auto fail = [&](const char* what) { msg = std::string(who) + ": " + what; g_last_error = msg.c_str(); return GSR_ERR_INVALID_ARGUMENT; };
    if (!m) return fail("null descriptor");
    if (m->in_dim < 16 || m->in_dim > 128 || m->in_dim % 16) return fail("in_dim must be a multiple of 16 in 16..128");
    if (!m->W0 || !m->b0) return fail("null W0 / b0");
    static const int od[3] = {3, 3, 4}, oo[3] = {0, 3, 6};
    w->W0 = m->W0; w->b0 = m->b0; w->in_dim = m->in_dim;
    for (int j = 0; j < 3; j++) {
        if (!m->W1[j] || !m->b1[j] || !m->W2[j] || !m->b2[j]) return fail("null head weights");
        w->W1[j] = m->W1[j]; w->b1[j] = m->b1[j]; w->W2[j] = m->W2[j]; w->b2[j] = m->b2[j];
        w->out_dim[j] = od[j]; w->out_off[j] = oo[j];
    }
    return 0;
}

static dim3 mlp_grid(int64_t n)
{
    const int64_t tiles = (n + MLP_TILE - 1) / MLP_TILE;
    return dim3((unsigned)std::min<int64_t>(tiles, 256));        // persistent: one block per CU (the weights live in its LDS)
}

constexpr int MLP_BWD_BLOCKS = 256;      // persistent: one block per CU (103 KB of LDS each)

int gsr_deform_mlp_forward(const gsr_deform_mlp* mlp, int64_t n, const float* features, float* out, void* stream_)
{
    MlpWeights w;
    if (int rc = mlp_fill(mlp, &w, "gsr_deform_mlp_forward")) return rc;
    if (n < 0 || (n > 0 && (!features || !out))) { g_last_error = "gsr_deform_mlp_forward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n == 0) return 0;
    // round 6: the bf16-split kernel (gs_mlp.h: three terms per operand, six products, weights stationary in registers) for the widths the
    // shipped networks use, two row tiles per block (two blocks per CU: 1.37 ms at 4 M rows; four row tiles, one block per CU: 1.65); every
    // other width: the fp32-MFMA kernel of rounds 1-5
    const int nt = w.in_dim / 16;
    if (nt == 2 || nt == 4 || nt == 8) {
        static std::atomic<unsigned long long> attr_set[3];
#define GSR_MLP3_LAUNCH(NT, SLOT)                                                                                                                 \
        do {                                                                                                                                      \
            using L = Mlp3Layout<NT, 2>;                                                                                                          \
            { const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(deform_mlp_fwd3_kernel<NT, 2>), L::BYTES, attr_set[SLOT]); if (rc) return rc; } \
            const int64_t tiles = (n + L::R - 1) / L::R;                                                                                          \
            hipLaunchKernelGGL((deform_mlp_fwd3_kernel<NT, 2>), dim3((unsigned)std::min<int64_t>(tiles, 256 * 2)), dim3(MLP3_THREADS), L::BYTES,  \
                               (hipStream_t)stream_, n, features, w, out);                                                                        \
        } while (0)
        if (nt == 2) GSR_MLP3_LAUNCH(2, 0); else if (nt == 4) GSR_MLP3_LAUNCH(4, 1); else GSR_MLP3_LAUNCH(8, 2);
#undef GSR_MLP3_LAUNCH
        GSR_HIP_CHECK(hipGetLastError());
        return 0;
    }
    switch (w.in_dim / 16) {
#define GSR_MLPF_CASE(NT) case NT: hipLaunchKernelGGL((deform_mlp_fwd_kernel<NT>), mlp_grid(n), dim3(MLP_BLOCK), 0, (hipStream_t)stream_, n, features, w, out); break;
        GSR_MLPF_CASE(1) GSR_MLPF_CASE(2) GSR_MLPF_CASE(3) GSR_MLPF_CASE(4) GSR_MLPF_CASE(5) GSR_MLPF_CASE(6) GSR_MLPF_CASE(7) GSR_MLPF_CASE(8)
#undef GSR_MLPF_CASE
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t gsr_deform_mlp_grad_count(int in_dim)
{
    static const int od[3] = {3, 3, 4};
    return (size_t)mlp_grad_layout(in_dim, od).total;
}

size_t gsr_deform_mlp_workspace_size(int in_dim)
{
    return (size_t)MLP_BWD_BLOCKS * gsr_deform_mlp_grad_count(in_dim) * sizeof(float) + 256;
}

size_t gsr_row_mask_workspace_size(int V, int64_t n)
{
    if (V < 1 || n < 0) return 256;
    return (size_t)V * (size_t)((n + ROWMASK_BLOCK - 1) / ROWMASK_BLOCK) * sizeof(uint32_t) + 256;
}

int gsr_row_mask(int V, int64_t n, int width, const float* g, uint32_t* view_mask, int32_t* rows, int32_t* n_rows, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 1 || V > 32 || n < 0 || width < 1 || (int64_t)V * n >= ((int64_t)1 << 31) || !n_rows || !workspace || (n > 0 && (!g || !view_mask || !rows))) {
        g_last_error = "gsr_row_mask: invalid argument (1 <= V <= 32, V n < 2^31, non-null pointers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) { GSR_HIP_CHECK(hipMemsetAsync(n_rows, 0, sizeof(int32_t), stream)); return 0; }
    const int nb = (int)((n + ROWMASK_BLOCK - 1) / ROWMASK_BLOCK);
    uint32_t* counts = reinterpret_cast<uint32_t*>(workspace);
    hipLaunchKernelGGL(rowmask_count_kernel, dim3(nb), dim3(ROWMASK_BLOCK), 0, stream, V, n, width, g, view_mask, counts);
    hipLaunchKernelGGL(rowmask_scan_kernel, dim3(1), dim3(1024), 0, stream, counts, V * nb, n_rows);
    hipLaunchKernelGGL(rowmask_list_kernel, dim3(nb), dim3(ROWMASK_BLOCK), 0, stream, V, n, (const uint32_t*)view_mask, (const uint32_t*)counts, rows);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_deform_mlp_backward(const gsr_deform_mlp* mlp, int64_t n, const float* features, const float* dout, float* dfeatures,
                            float* grads, char* workspace, void* stream_)
{
    return gsr_deform_mlp_backward_rows(mlp, n, features, dout, dfeatures, grads, workspace, nullptr, nullptr, stream_);
}

int gsr_deform_mlp_backward_rows(const gsr_deform_mlp* mlp, int64_t n, const float* features, const float* dout, float* dfeatures,
                                 float* grads, char* workspace, const int32_t* rows, const int32_t* n_rows, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    MlpWeights w;
    if (int rc = mlp_fill(mlp, &w, "gsr_deform_mlp_backward")) return rc;
    if ((rows != nullptr) != (n_rows != nullptr)) { g_last_error = "gsr_deform_mlp_backward_rows: rows and n_rows go together"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n < 0 || !grads || !workspace || (n > 0 && (!features || !dout || !dfeatures))) {
        g_last_error = "gsr_deform_mlp_backward: null / invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const int total = (int)gsr_deform_mlp_grad_count(w.in_dim);
    if (n == 0) { GSR_HIP_CHECK(hipMemsetAsync(grads, 0, (size_t)total * sizeof(float), stream)); return 0; }
    const int blocks = (int)std::min<int64_t>(MLP_BWD_BLOCKS, (n + MLPB_TILE - 1) / MLPB_TILE);
    float* partial = reinterpret_cast<float*>(workspace);
    switch (w.in_dim / 16) {
#define GSR_MLPB_CASE(NT) case NT: hipLaunchKernelGGL((deform_mlp_bwd_kernel<NT>), dim3(blocks), dim3(MLPB_BLOCK), 0, stream, n, features, dout, w, dfeatures, partial, rows, n_rows); break;
        GSR_MLPB_CASE(1) GSR_MLPB_CASE(2) GSR_MLPB_CASE(3) GSR_MLPB_CASE(4) GSR_MLPB_CASE(5) GSR_MLPB_CASE(6) GSR_MLPB_CASE(7) GSR_MLPB_CASE(8)
#undef GSR_MLPB_CASE
    }
    hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, blocks, total, (const float*)partial, grads);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- fp32-accurate dense layers on the bf16 matrix cores (include/dense_layers.h) ---------------------------------------------------------
static inline int round_up_int(int v, int m) { return (v + m - 1) / m * m; }

size_t gsr_dense_planes_size(int rows, int cols)
{
    if (rows < 1 || cols < 1) return 0;
    return (size_t)3 * round_up_int(rows, DENSE_BN) * round_up_int(cols, DENSE_BK) * sizeof(unsigned short);
}

int gsr_dense_split(int N, int K, const float* W, int ldw, int k0, int transposed, void* planes, void* stream_)
{
    if (N < 1 || K < 1 || !W || !planes || ldw < k0 + K || k0 < 0) { g_last_error = "gsr_dense_split: invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    const int rows = transposed ? K : N, cols = transposed ? N : K;
    const int rows_pad = round_up_int(rows, DENSE_BN), cols_pad = round_up_int(cols, DENSE_BK);
    const int64_t count = (int64_t)rows_pad * cols_pad;
    hipLaunchKernelGGL(dense_split_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, N, K, W, ldw, k0, transposed ? 1 : 0,
                       reinterpret_cast<unsigned short*>(planes), rows_pad, cols_pad);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static int dense_forward_launch(const char* who, int M, int N, int K, const float* X, int ldx, const float* gate, int ldgate, const void* planes, const float* bias,
                                int relu, float* Y, int ldy, const float* mask, int ldmask, float* colsum_out, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || N < 1 || K < 1 || !planes || (M > 0 && (!X || !Y)) || ldx < K || ldy < N || (gate && ldgate < K) || (mask && ldmask < N)) {
        g_last_error = std::string(who) + ": invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) {
        if (colsum_out) GSR_HIP_CHECK(hipMemsetAsync(colsum_out, 0, (size_t)N * sizeof(float), stream));
        return 0;
    }
    const int Npad = round_up_int(N, DENSE_BN), Kpad = round_up_int(K, DENSE_BK);
    const int vec = (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(X) % 16 == 0) && (!gate || ((ldgate % 4 == 0) && reinterpret_cast<uintptr_t>(gate) % 16 == 0));
    // 16-byte output stores through an LDS transposition when every row piece is whole and aligned (the trunk's layers), else element stores
    const int vec_out = (N % 4 == 0) && (ldy % 4 == 0) && (reinterpret_cast<uintptr_t>(Y) % 16 == 0) && (!bias || reinterpret_cast<uintptr_t>(bias) % 16 == 0) &&
                        (!mask || ((ldmask % 4 == 0) && reinterpret_cast<uintptr_t>(mask) % 16 == 0));
    if (colsum_out && (!vec_out || !workspace || (reinterpret_cast<uintptr_t>(workspace) % 16))) {
        g_last_error = std::string(who) + ": the column sums need N % 4 == 0, 16-byte aligned rows of Y / mask and a 16-byte aligned workspace"; return GSR_ERR_INVALID_ARGUMENT;
    }
    float* partial = colsum_out ? reinterpret_cast<float*>(workspace) : nullptr;
    // full-width outputs (the network's layers): one block of eight waves per CU, two LDS stages (dense_fwd8_kernel); otherwise the
    // 128-column kernel
    if (vec_out && N % DENSE8_BN == 0) {
        const int bt8 = dense8_row_tiles(M, N / DENSE8_BN);
        const dim3 grid8((unsigned)((M + 16 * bt8 - 1) / (16 * bt8)), (unsigned)(N / DENSE8_BN));
        Dense8Layer L;
        L.X = X; L.gate = gate; L.planes = reinterpret_cast<const unsigned short*>(planes); L.bias = bias; L.Y = Y; L.mask = mask; L.colsum = partial;
        L.N = N; L.K = K; L.ldx = ldx; L.ldgate = ldgate; L.Npad = Npad; L.Kpad = Kpad; L.relu = relu ? 1 : 0; L.ldy = ldy; L.vec = vec ? 1 : 0; L.ldmask = ldmask;
        static std::atomic<unsigned long long> attr_set[DENSE_MAX_BT + 1];
#define GSR_DENSE8_LAUNCH(BT)                                                                                                                          \
        case BT:                                                                                                                                       \
            { const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(dense_fwd8_kernel<BT>), DENSE8_LDS_BYTES, attr_set[BT]); if (rc) return rc; } \
            hipLaunchKernelGGL(dense_fwd8_kernel<BT>, grid8, dim3(DENSE8_THREADS), DENSE8_LDS_BYTES, stream, M, L);                                    \
            break;
        switch (bt8) {
            GSR_DENSE8_LAUNCH(2) GSR_DENSE8_LAUNCH(3) GSR_DENSE8_LAUNCH(4) GSR_DENSE8_LAUNCH(5) GSR_DENSE8_LAUNCH(6) GSR_DENSE8_LAUNCH(7)
            GSR_DENSE8_LAUNCH(8) GSR_DENSE8_LAUNCH(9) GSR_DENSE8_LAUNCH(10)
        }
#undef GSR_DENSE8_LAUNCH
        if (colsum_out) hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, stream, (int)grid8.x, N, (const float*)partial, colsum_out);
        GSR_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const int bt = dense_row_tiles(M, Npad / DENSE_BN);
    const dim3 grid((unsigned)((M + 16 * bt - 1) / (16 * bt)), (unsigned)(Npad / DENSE_BN));
    hipLaunchKernelGGL(dense_fwd_kernel, grid, dim3(DENSE_THREADS), 0, stream, M, N, K, X, ldx, gate, ldgate,
                       reinterpret_cast<const unsigned short*>(planes), Npad, Kpad, bias, relu ? 1 : 0, Y, ldy, vec ? 1 : 0, vec_out ? 1 : 0, bt, mask, ldmask, partial);
    if (colsum_out) hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, stream, (int)grid.x, N, (const float*)partial, colsum_out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_dense_forward(int M, int N, int K, const float* X, int ldx, const float* gate, int ldgate, const void* planes, const float* bias, int relu,
                      float* Y, int ldy, void* stream_)
{
    return dense_forward_launch("gsr_dense_forward", M, N, K, X, ldx, gate, ldgate, planes, bias, relu, Y, ldy, nullptr, 0, nullptr, nullptr, stream_);
}

size_t gsr_dense_backward_input_workspace_size(int M, int N)
{
    if (M < 1 || N < 1) return 256;
    return (size_t)((M + 31) / 32) * (size_t)N * sizeof(float) + 256;        // (at least two row tiles of 16 per block)
}

int gsr_dense_backward_input(int M, int N, int K, const float* G, int ldg, const void* planes_t, const float* mask, int ldmask, float* dX, int lddx,
                             float* dbias, char* workspace, void* stream_)
{
    return dense_forward_launch("gsr_dense_backward_input", M, N, K, G, ldg, nullptr, 0, planes_t, nullptr, 0, dX, lddx, mask, ldmask, dbias, workspace, stream_);
}

// workspace of gsr_dense_chain: per product the column sums of its row bands [ceil(M / 32), N], each product's starting on a multiple of 256 bytes
struct DenseChainWs { float* partial; size_t per_op_floats, bytes; };
static DenseChainWs dense_chain_layout(int M, int N, int count, const char* workspace)
{
    Carver c(workspace, 256);
    const size_t per_op_floats = M < 1 || N < 1 || count < 1 ? 0 : c.up((size_t)((M + 31) / 32) * (size_t)N * sizeof(float)) / sizeof(float);
    return {c.take<float>((size_t)std::max(count, 0) * per_op_floats), per_op_floats, c.bytes()};
}
size_t gsr_dense_chain_workspace_size(int M, int N, int count) { return dense_chain_layout(M, N, count, nullptr).bytes; }

int gsr_dense_chain(int M, int N, int count, const gsr_dense_chain_op* ops, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || N < 1 || N != DENSE8_BN || count < 1 || count > DENSE8_CHAIN_MAX || !ops) {
        g_last_error = "gsr_dense_chain: 1..8 products of 256 output columns each"; return GSR_ERR_INVALID_ARGUMENT;
    }
    bool sums = false;
    for (int l = 0; l < count; l++) {
        const gsr_dense_chain_op& q = ops[l];
        const bool aligned = (q.ldx % 4 == 0) && (q.ldy % 4 == 0) && !(reinterpret_cast<uintptr_t>(q.X) % 16) && !(reinterpret_cast<uintptr_t>(q.Y) % 16) &&
                             (!q.bias || !(reinterpret_cast<uintptr_t>(q.bias) % 16)) && (!q.mask || ((q.ldmask % 4 == 0) && !(reinterpret_cast<uintptr_t>(q.mask) % 16)));
        if (q.K < 1 || !q.planes || (M > 0 && (!q.X || !q.Y)) || q.ldx < q.K || q.ldy < N || (q.mask && q.ldmask < N) || !aligned) {
            g_last_error = "gsr_dense_chain: invalid product (16-byte aligned rows of X / Y / mask, ldx >= K, ldy >= 256)"; return GSR_ERR_INVALID_ARGUMENT;
        }
        sums = sums || q.dbias;
    }
    if (sums && (!workspace || (reinterpret_cast<uintptr_t>(workspace) % 16))) { g_last_error = "gsr_dense_chain: the bias gradients need a 16-byte aligned workspace"; return GSR_ERR_INVALID_ARGUMENT; }
    if (M == 0) {
        for (int l = 0; l < count; l++) if (ops[l].dbias) GSR_HIP_CHECK(hipMemsetAsync(ops[l].dbias, 0, (size_t)N * sizeof(float), stream));
        return 0;
    }
    const int bt = dense8_row_tiles(M, 1);
    const unsigned blocks = (unsigned)((M + 16 * bt - 1) / (16 * bt));
    const DenseChainWs w = dense_chain_layout(M, N, count, workspace);
    Dense8Chain c;
    c.M = M; c.count = count;
    float* partial[DENSE8_CHAIN_MAX];
    for (int l = 0; l < count; l++) {
        const gsr_dense_chain_op& q = ops[l];
        Dense8Layer& L = c.layer[l];
        partial[l] = q.dbias ? w.partial + (size_t)l * w.per_op_floats : nullptr;
        L.X = q.X; L.gate = nullptr; L.planes = reinterpret_cast<const unsigned short*>(q.planes); L.bias = q.bias; L.Y = q.Y; L.mask = q.mask; L.colsum = partial[l];
        L.N = N; L.K = q.K; L.ldx = q.ldx; L.ldgate = 0; L.Npad = round_up_int(N, DENSE_BN); L.Kpad = round_up_int(q.K, DENSE_BK); L.relu = q.relu ? 1 : 0;
        L.ldy = q.ldy; L.vec = 1; L.ldmask = q.ldmask;
    }
    static std::atomic<unsigned long long> attr_set[DENSE_MAX_BT + 1];
#define GSR_CHAIN8_LAUNCH(BT)                                                                                                                          \
    case BT:                                                                                                                                           \
        { const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(dense_chain8_kernel<BT>), DENSE8_LDS_BYTES, attr_set[BT]); if (rc) return rc; } \
        hipLaunchKernelGGL(dense_chain8_kernel<BT>, dim3(blocks), dim3(DENSE8_THREADS), DENSE8_LDS_BYTES, stream, c);                                  \
        break;
    switch (bt) {
        GSR_CHAIN8_LAUNCH(2) GSR_CHAIN8_LAUNCH(3) GSR_CHAIN8_LAUNCH(4) GSR_CHAIN8_LAUNCH(5) GSR_CHAIN8_LAUNCH(6) GSR_CHAIN8_LAUNCH(7)
        GSR_CHAIN8_LAUNCH(8) GSR_CHAIN8_LAUNCH(9) GSR_CHAIN8_LAUNCH(10)
    }
#undef GSR_CHAIN8_LAUNCH
    for (int l = 0; l < count; l++)
        if (ops[l].dbias) hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, stream, (int)blocks, N, (const float*)partial[l], ops[l].dbias);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_dense_split_many(int count, const gsr_dense_split_item* items, void* stream_)
{
    if (count < 0 || count > DENSE_SPLIT_MAX || (count > 0 && !items)) { g_last_error = "gsr_dense_split_many: 0 <= count <= 24 items"; return GSR_ERR_INVALID_ARGUMENT; }
    if (count == 0) return 0;
    DenseSplitItems a;
    int64_t largest = 0;
    for (int i = 0; i < count; i++) {
        const gsr_dense_split_item& q = items[i];
        if (q.N < 1 || q.K < 1 || !q.W || !q.planes || q.k0 < 0 || q.ldw < q.k0 + q.K) { g_last_error = "gsr_dense_split_many: invalid item"; return GSR_ERR_INVALID_ARGUMENT; }
        const int rows = q.transposed ? q.K : q.N, cols = q.transposed ? q.N : q.K;
        DenseSplitItem& d = a.item[i];
        d.W = q.W; d.planes = reinterpret_cast<unsigned short*>(q.planes); d.N = q.N; d.K = q.K; d.ldw = q.ldw; d.k0 = q.k0; d.transposed = q.transposed ? 1 : 0;
        d.rows_pad = round_up_int(rows, DENSE_BN); d.cols_pad = round_up_int(cols, DENSE_BK);
        largest = std::max(largest, (int64_t)d.rows_pad * d.cols_pad);
    }
    const unsigned bx = (unsigned)std::min<int64_t>((largest + 255) / 256, 128);
    hipLaunchKernelGGL(dense_split_many_kernel, dim3(bx, (unsigned)count), dim3(256), 0, (hipStream_t)stream_, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static void dense_wgrad_plan(int M, int N, int K, int* slices, int* rows_per_slice)
{
    const int tiles = ((N + DENSE_BM - 1) / DENSE_BM) * ((K + DENSE_BN - 1) / DENSE_BN);
    int s = std::max(1, 512 / std::max(1, tiles));                             // ~two blocks per CU
    s = std::min(s, std::max(1, (M + 4 * DENSE_WG_ROWS - 1) / (4 * DENSE_WG_ROWS)));   // at least four steps per slice
    const int rps = round_up_int((M + s - 1) / s, DENSE_WG_ROWS);
    *rows_per_slice = std::max(rps, DENSE_WG_ROWS);
    *slices = std::max(1, (M + *rows_per_slice - 1) / *rows_per_slice);
}

// workspace of gsr_dense_wgrad and gsr_dense_wgrad_many: the slices' partial products, `floats` of them, at a base the call aligns to 256 bytes
struct WgradWs { float* partial; size_t bytes; };
static WgradWs wgrad_layout(size_t floats, const char* workspace)
{
    Carver c(workspace, 256, true);
    return {c.take<float>(floats), c.bytes()};
}
static WgradWs dense_wgrad_layout(int M, int N, int K, int slices, const char* workspace)         // slices: of dense_wgrad_plan
{
    return wgrad_layout(M < 1 || N < 1 || K < 1 ? 0 : (size_t)slices * N * K, workspace);
}
size_t gsr_dense_wgrad_workspace_size(int M, int N, int K)
{
    int slices, rps;
    dense_wgrad_plan(M, N, K, &slices, &rps);
    return dense_wgrad_layout(M, N, K, slices, nullptr).bytes;
}

int gsr_dense_wgrad(int M, int N, int K, const float* G, int ldg, const float* gate, int ldgate, const float* X, int ldx, float* dW, int lddw,
                    char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || N < 1 || K < 1 || !dW || lddw < K || (M > 0 && (!G || !X || !workspace)) || ldg < N || ldx < K || (gate && ldgate < N)) {
        g_last_error = "gsr_dense_wgrad: invalid argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) { GSR_HIP_CHECK(hipMemset2DAsync(dW, (size_t)lddw * sizeof(float), 0, (size_t)K * sizeof(float), (size_t)N, stream)); return 0; }
    int slices, rps;
    dense_wgrad_plan(M, N, K, &slices, &rps);
    float* partial = dense_wgrad_layout(M, N, K, slices, workspace).partial;
    const dim3 grid((unsigned)((N + DENSE_BM - 1) / DENSE_BM), (unsigned)((K + DENSE_BN - 1) / DENSE_BN), (unsigned)slices);
    hipLaunchKernelGGL(dense_wgrad_kernel, grid, dim3(DENSE_THREADS), 0, stream, M, N, K, G, ldg, gate, ldgate, X, ldx, rps, partial);
    hipLaunchKernelGGL(dense_wgrad_sum_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, stream, slices, N * K, (const float*)partial, K, dW, lddw);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// several weight gradients over the same rows in one launch (gs_dense.h, round 6)
static int dense_wgrad_many_plan(int M, int count, const gsr_dense_wgrad_item* items, DenseWgradItems* out, int* slices, int* rows_per_slice)
{
    if (count < 1 || count > DENSE_WGM_MAX || !items) return -1;
    int tiles = 0;
    for (int i = 0; i < count; i++) {
        const gsr_dense_wgrad_item& q = items[i];
        if (q.N < 1 || q.K < 1 || q.ldg < q.N || q.ldx < q.K || q.lddw < q.K) return -1;
        if (out) {
            DenseWgradItem& d = out->item[i];
            d.G = q.G; d.X = q.X; d.dW = q.dW; d.ldg = q.ldg; d.ldx = q.ldx; d.lddw = q.lddw; d.N = q.N; d.K = q.K;
            d.tiles_k = (q.K + DENSE_BN - 1) / DENSE_BN; d.tile0 = tiles;
            d.vec = (q.N % 4 == 0 && q.K % 4 == 0 && q.ldg % 4 == 0 && q.ldx % 4 == 0 && reinterpret_cast<uintptr_t>(q.G) % 16 == 0 && reinterpret_cast<uintptr_t>(q.X) % 16 == 0) ? 1 : 0;
        }
        tiles += ((q.N + DENSE_BM - 1) / DENSE_BM) * ((q.K + DENSE_BN - 1) / DENSE_BN);
    }
    if (out) { out->count = count; out->total_tiles = tiles; }
    // every block resident at once (512 blocks: two per CU), at least four 32-row steps per slice
    int s = std::max(1, 512 / std::max(1, tiles));
    s = std::min(s, std::max(1, (M + 4 * DENSE_WG_ROWS - 1) / (4 * DENSE_WG_ROWS)));
    const int rps = std::max(DENSE_WG_ROWS, round_up_int((std::max(M, 1) + s - 1) / s, DENSE_WG_ROWS));
    *rows_per_slice = rps;
    *slices = std::max(1, (M + rps - 1) / rps);
    return tiles;
}

static WgradWs dense_wgrad_many_layout(int M, int tiles, int slices, const char* workspace)      // tiles, slices: of dense_wgrad_many_plan
{
    return wgrad_layout(tiles < 0 || M < 1 ? 0 : (size_t)slices * tiles * (DENSE_BM * DENSE_BN), workspace);
}
size_t gsr_dense_wgrad_many_workspace_size(int M, int count, const gsr_dense_wgrad_item* items)
{
    int slices = 0, rps = 0;
    const int tiles = dense_wgrad_many_plan(M, count, items, nullptr, &slices, &rps);
    return dense_wgrad_many_layout(M, tiles, slices, nullptr).bytes;
}

int gsr_dense_wgrad_many(int M, int count, const gsr_dense_wgrad_item* items, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DenseWgradItems t;
    memset(&t, 0, sizeof(t));
    int slices, rps;
    const int tiles = M < 0 ? -1 : dense_wgrad_many_plan(M, count, items, &t, &slices, &rps);
    bool ok = tiles > 0;
    for (int i = 0; ok && i < count; i++) ok = items[i].dW && (M == 0 || (items[i].G && items[i].X));
    if (!ok || (M > 0 && !workspace)) {
        g_last_error = "gsr_dense_wgrad_many: invalid argument (1..12 items, ldg >= N, ldx >= K, lddw >= K, non-null operands and workspace)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) {
        for (int i = 0; i < count; i++)
            GSR_HIP_CHECK(hipMemset2DAsync(items[i].dW, (size_t)items[i].lddw * sizeof(float), 0, (size_t)items[i].K * sizeof(float), (size_t)items[i].N, stream));
        return 0;
    }
    float* partial = dense_wgrad_many_layout(M, tiles, slices, workspace).partial;
    hipLaunchKernelGGL(dense_wgrad_many_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(DENSE_THREADS), 0, stream, M, t, rps, partial);
    hipLaunchKernelGGL(dense_wgrad_many_sum_kernel, dim3((unsigned)tiles, 16), dim3(256), 0, stream, t, slices, (const float*)partial);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_trunk_forward(const gsr_trunk* t, int R, const float* emb, float* const* outs, const int* ldo, float* heads, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!t || R < 0 || t->E < 1 || t->E > TR_EPAD || t->n_head_outputs < 1 || t->n_head_outputs > 16 || !outs || !ldo || (R > 0 && (!emb || !heads))) {
        g_last_error = "gsr_trunk_forward: invalid argument (embedding width 1..96, 1..16 head outputs)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    TrunkArgs a{};
    a.R = R; a.E = t->E; a.NH = t->n_head_outputs; a.emb = emb; a.heads = heads;
    for (int k = 0; k < 10; k++) { if (!t->planes[k]) { g_last_error = "gsr_trunk_forward: null weight planes"; return GSR_ERR_INVALID_ARGUMENT; } a.planes[k] = reinterpret_cast<const unsigned short*>(t->planes[k]); }
    for (int k = 0; k < 9; k++) { if (!t->bias[k] || reinterpret_cast<uintptr_t>(t->bias[k]) % 16) { g_last_error = "gsr_trunk_forward: null / unaligned bias"; return GSR_ERR_INVALID_ARGUMENT; } a.bias[k] = t->bias[k]; }
    for (int l = 0; l < TR_LAYERS; l++) {
        if (!outs[l] || ldo[l] < TR_W || ldo[l] % 4 || reinterpret_cast<uintptr_t>(outs[l]) % 16) { g_last_error = "gsr_trunk_forward: layer outputs must be 16-byte aligned rows of >= 256 floats"; return GSR_ERR_INVALID_ARGUMENT; }
        a.outs[l] = outs[l]; a.ldo[l] = ldo[l];
    }
    if (R == 0) return 0;
    static std::atomic<unsigned long long> attr_set;
    { const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(trunk_fwd_kernel), TR_LDS_BYTES, attr_set); if (rc) return rc; }
    hipLaunchKernelGGL(trunk_fwd_kernel, dim3((unsigned)((R + TR_BM - 1) / TR_BM)), dim3(256), TR_LDS_BYTES, stream, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- SC-GS control nodes (include/control_nodes.h) ------------------------------------------------------------------------------
int gsr_knn_points_batch(int64_t B, int64_t n, int64_t m, int D, int K, const float* p1, const float* p2, float* dist2, int64_t* idx, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (B < 0 || B > 65535 || n < 0 || m < 0 || D < 1 || D > GSR_KNN_MAX_DIM || K < 1 || K > GSR_KNN_MAX_K || (B > 0 && n > 0 && (!p1 || !dist2 || !idx)) ||
        (B > 0 && m > 0 && !p2)) {
        g_last_error = "gsr_knn_points_batch: null / invalid argument (0 <= B <= 65535, 1 <= D <= 32, 1 <= K <= 32)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (B == 0 || n == 0) return 0;
    if (D <= 4 && K > 4 && m <= 64 * 16) {            // small candidate sets, longer lists: one wave per query, all batch elements in one launch
        const dim3 grid((unsigned)((n + NODE_BLOCK / 64 - 1) / (NODE_BLOCK / 64)), (unsigned)B), block(NODE_BLOCK);
#define GSR_KNNW(C) hipLaunchKernelGGL((knn_points3_wave_kernel<C>), grid, block, 0, stream, n, m, D, K, p1, p2, dist2, idx)
        if (m <= 64 * 4) GSR_KNNW(4); else if (m <= 64 * 8) GSR_KNNW(8); else GSR_KNNW(16);
#undef GSR_KNNW
        GSR_HIP_CHECK(hipGetLastError());
        return 0;
    }
    for (int64_t b = 0; b < B; b++) {
        const int rc = gsr_knn_points(n, m, D, K, p1 + b * n * D, p2 ? p2 + b * m * D : p2, dist2 + b * n * K, idx + b * n * K, stream_);
        if (rc < 0) return rc;
    }
    return 0;
}

int gsr_knn_points(int64_t n, int64_t m, int D, int K, const float* p1, const float* p2, float* dist2, int64_t* idx, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || m < 0 || D < 1 || D > GSR_KNN_MAX_DIM || K < 1 || K > GSR_KNN_MAX_K || (n > 0 && (!p1 || !dist2 || !idx)) || (m > 0 && !p2)) {
        g_last_error = "gsr_knn_points: null / invalid argument (1 <= D <= 32, 1 <= K <= 32)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return 0;
    const int64_t rows = std::min<int64_t>((int64_t)(NODE_CHUNK * 3 / D), std::max<int64_t>(m, 1));
    const size_t lds = (size_t)rows * D * sizeof(float);
    const dim3 grid((unsigned)((n + NODE_BLOCK - 1) / NODE_BLOCK)), block(NODE_BLOCK);
#define GSR_KNN_LAUNCH(DMAX, KMAX) hipLaunchKernelGGL((knn_points_kernel<DMAX, KMAX>), grid, block, lds, stream, n, m, D, K, p1, p2, dist2, idx)
#define GSR_KNN_K(DMAX) do { if (K <= 4) GSR_KNN_LAUNCH(DMAX, 4); else if (K <= 8) GSR_KNN_LAUNCH(DMAX, 8); else if (K <= 16) GSR_KNN_LAUNCH(DMAX, 16); else GSR_KNN_LAUNCH(DMAX, 32); } while (0)
    if (D <= 4) {
#define GSR_KNN3(KMAX, EXACT) hipLaunchKernelGGL((knn_points3_kernel<KMAX, EXACT>), grid, block, 0, stream, n, m, D, K, p1, p2, dist2, idx)
        switch (K) {
        case 1: GSR_KNN3(1, true); break;
        case 2: GSR_KNN3(2, true); break;
        case 3: GSR_KNN3(3, true); break;
        case 4: GSR_KNN3(4, true); break;
        default: if (K <= 8) GSR_KNN3(8, false); else if (K <= 16) GSR_KNN3(16, false); else GSR_KNN3(32, false);
        }
#undef GSR_KNN3
    } else if (D <= 8) GSR_KNN_K(8); else GSR_KNN_K(32);
#undef GSR_KNN_K
#undef GSR_KNN_LAUNCH
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static int node_blend_check(const gsr_node_blend* a, const char* who)
{
    static thread_local std::string msg;
    auto fail = [&](const char* what) { msg = std::string(who) + ": " + what; g_last_error = msg.c_str(); return GSR_ERR_INVALID_ARGUMENT; };
    if (!a) return fail("null descriptor");
    if (a->n < 0 || a->m < 1) return fail("n < 0 or no control nodes");
    if (a->K < 1 || a->K > GSR_BLEND_MAX_K) return fail("K outside 1..8");
    if (a->node_stride < 3) return fail("node_stride < 3");
    if (a->n > 0 && !a->x) return fail("null x");
    if (!a->nodes || !a->node_radius) return fail("null nodes / node_radius");
    if (a->node_trans && (!a->node_rot || !a->node_scale)) return fail("node_trans without node_rot / node_scale");
    if (a->node_trans && a->local_frame && !a->node_frame && !a->node_local_rotation) return fail("local_frame without node_frame / node_local_rotation");
    if (a->attr_stride < 0 || a->grad_stride < 0 || (a->attr_stride > 0 && (a->attr_stride < 4 || a->node_frame)) || (a->grad_stride > 0 && a->grad_stride < 4))
        return fail("attr_stride / grad_stride: 0 (packed) or >= 4 floats per node, and no node_frame with strided attributes");
    return 0;
}

int gsr_node_blend_forward(const gsr_node_blend* a, float* nn_weight, float* nn_dist, int64_t* nn_idx, float* d_xyz, float* d_rotation,
                           float* d_scaling, void* stream_)
{
    return gsr_node_blend_forward_batch(a, 1, nn_weight, nn_dist, nn_idx, d_xyz, d_rotation, d_scaling, stream_);
}

int gsr_node_blend_forward_batch(const gsr_node_blend* a, int B, float* nn_weight, float* nn_dist, int64_t* nn_idx, float* d_xyz, float* d_rotation,
                                 float* d_scaling, void* stream_)
{
    if (int rc = node_blend_check(a, "gsr_node_blend_forward")) return rc;
    if (B < 1 || B > 65535 || (B > 1 && !a->node_trans)) { g_last_error = "gsr_node_blend_forward_batch: 1 <= B <= 65535, B > 1 needs node attributes"; return GSR_ERR_INVALID_ARGUMENT; }
    if (a->n == 0) return 0;
    if (!nn_weight || !nn_dist || !nn_idx || (a->node_trans && (!d_xyz || !d_rotation || !d_scaling))) {
        g_last_error = "gsr_node_blend_forward: null output"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid((unsigned)((a->n + NODE_BLOCK - 1) / NODE_BLOCK), (unsigned)B), block(NODE_BLOCK);
#define GSR_BLEND_FWD(KMAX, EXACT) hipLaunchKernelGGL((node_blend_fwd_kernel<KMAX, EXACT>), grid, block, 0, (hipStream_t)stream_, *a, nn_weight, nn_dist, nn_idx, d_xyz, d_rotation, d_scaling)
    switch (a->K) {
    case 1: GSR_BLEND_FWD(1, true); break;
    case 2: GSR_BLEND_FWD(2, true); break;
    case 3: GSR_BLEND_FWD(3, true); break;
    case 4: GSR_BLEND_FWD(4, true); break;
    default: GSR_BLEND_FWD(GSR_BLEND_MAX_K, false);
    }
#undef GSR_BLEND_FWD
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static int node_bwd_blocks(int64_t n) { return (int)std::min<int64_t>(256, std::max<int64_t>(1, (n + NODE_BLOCK - 1) / NODE_BLOCK)); }

static size_t node_ws_floats(int64_t n, int32_t m)      // per batch element: block partials + the summed row, a multiple of 64 floats
{
    const size_t rows = m <= NODE_LDS_MAX ? (size_t)node_bwd_blocks(n) : 1;
    const size_t atomics_route = (rows + 1) * (size_t)m * NODE_GRAD;
    const size_t ordered_route = ((size_t)n * NODE_DET_MAX_K + (size_t)m) * NODE_GRAD;        // per-(Gaussian, k) contributions + the summed row
    return (std::max(atomics_route, ordered_route) + 63) & ~size_t(63);
}
static int index_csr_epad(int E) { return round_up_int(E, CSR_REG_TRIP); }

/* ---- deterministic scatter-add through an index array (include/control_nodes.h) ------------------------------------------------------ */
// workspace of gsr_index_csr, read again by gsr_segment_sum: cursor [S] | order [S, E] with seg [S, Nv] {begin, count} right behind it | the
// sets packed to 16 bits [S, Epad] (small sets only)
struct IndexCsrWs { int *cursor, *order, *seg; unsigned short* packed; size_t bytes; };
static IndexCsrWs index_csr_layout(int S, int E, int Nv, const char* workspace)
{
    const size_t s = (size_t)std::max(S, 0), e = (size_t)std::max(E, 0), nv = (size_t)std::max(Nv, 0);
    Carver c(workspace, 256, true);
    int* const cursor = c.take<int>(s), * const order = c.take<int>(s * e + 2 * s * nv);
    return {cursor, order, order ? order + s * e : nullptr, c.take<unsigned short>(s * (size_t)index_csr_epad(E > 0 ? E : 1)), c.bytes()};
}
size_t gsr_index_csr_workspace_size(int S, int E, int Nv) { return index_csr_layout(S, E, Nv, nullptr).bytes; }

// workspace of the blend's backward pass: per batch element the block partials and the summed row | once per call (any batch size) the
// reverse lists of nn_idx, gsr_index_csr's workspace for one set
struct NodeBlendWs { float* partial; size_t stride; char* csr; size_t bytes; };
static NodeBlendWs node_blend_layout(int64_t n, int32_t m, int B, const char* workspace)
{
    Carver c(workspace, 256, true);
    NodeBlendWs w{};
    if (m >= 1 && B >= 1) {
        const int E = (int)std::min<int64_t>(n * NODE_DET_MAX_K, INT32_MAX / 2);
        w.stride = node_ws_floats(n, m);
        w.partial = c.take<float>((size_t)B * w.stride);
        w.csr = c.nested(index_csr_layout(1, E, m, nullptr).bytes);
    }
    w.bytes = c.bytes();
    return w;
}

size_t gsr_node_blend_workspace_size(int64_t n, int32_t m) { return node_blend_layout(n, m, 1, nullptr).bytes; }
size_t gsr_node_blend_workspace_size_batch(int64_t n, int32_t m, int B) { return node_blend_layout(n, m, B, nullptr).bytes; }

int gsr_index_csr(int S, int E, int Nv, const int64_t* idx, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (S < 1 || S > 65535 || E < 0 || Nv < 1 || !workspace || (E > 0 && !idx)) { g_last_error = "gsr_index_csr: invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    const auto [cursor, order, seg, packed, ws_bytes] = index_csr_layout(S, E, Nv, workspace);
    GSR_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)S * sizeof(int), stream));
    if (E >= 1 && E <= 20 * CSR_REG_TRIP && Nv < 65535) {          // small sets: packed to 16 bits, a wave holds the whole set in registers
        const int Epad = index_csr_epad(E);
        hipLaunchKernelGGL(index_csr_pack_kernel, dim3((unsigned)((Epad + 255) / 256), (unsigned)S), dim3(256), 0, stream, E, Epad, idx, packed);
        const dim3 grid((unsigned)((Nv + 3) / 4), (unsigned)S);
        if (Epad <= 10 * CSR_REG_TRIP) hipLaunchKernelGGL(index_csr_reg_kernel<10>, grid, dim3(256), 0, stream, E, Epad, Nv, (const unsigned short*)packed, order, seg, cursor);
        else hipLaunchKernelGGL(index_csr_reg_kernel<20>, grid, dim3(256), 0, stream, E, Epad, Nv, (const unsigned short*)packed, order, seg, cursor);
        GSR_HIP_CHECK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(index_csr_kernel, dim3((unsigned)((Nv + 3) / 4), (unsigned)S), dim3(256), 0, stream, E, Nv, idx, order, seg, cursor);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t gsr_node_embedding_workspace_size(int n, int M, int Fx, int Ft)
{
    return n >= 0 && M >= 0 && Fx >= 0 && Ft >= 0 ? ((size_t)M * 3 * (1 + 2 * Fx) + (size_t)n * (1 + 2 * Ft)) * sizeof(float) + 16 : 0;
}

int gsr_node_embedding(int n, int M, int Fx, int Ft, const float* nodes, int node_stride, const float* times, float* out, char* workspace, void* stream_)
{
    if (n < 0 || M < 0 || Fx < 0 || Fx > 24 || Ft < 0 || Ft > 24 || node_stride < 3 || ((size_t)n * M > 0 && (!nodes || !times || !out || !workspace))) {
        g_last_error = "gsr_node_embedding: invalid argument (0 <= frequencies <= 24, node_stride >= 3, no null buffers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const int Wx = 3 * (1 + 2 * Fx), Wt = 1 + 2 * Ft;
    const size_t total = (size_t)n * M * (Wx + Wt), small = (size_t)M * Wx + (size_t)n * Wt;
    if (total) {
        float* tables = reinterpret_cast<float*>(workspace);
        hipLaunchKernelGGL(node_embedding_tables_kernel, dim3((unsigned)((small + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, n, M, Fx, Ft, nodes, node_stride, times, tables);
        hipLaunchKernelGGL(node_embedding_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, n, M, Wx, Wt, (const float*)tables, out);
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t gsr_relu_backward_bias_workspace_size(int rows, int cols)
{
    return rows > 0 && cols > 0 ? (size_t)((rows + RELU_BAND - 1) / RELU_BAND) * (size_t)cols * sizeof(float) : 0;
}

int gsr_relu_backward_bias(int rows, int cols, const float* dY, const float* Y, float* G, float* dbias, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const bool cols_ok = cols == 64 || cols == 128 || cols == 256 || cols == 512 || cols == 1024;
    if (rows < 0 || !cols_ok || !dbias || (rows > 0 && (!dY || !Y || !G || !workspace))) {
        g_last_error = "gsr_relu_backward_bias: invalid argument (cols in {64, 128, 256, 512, 1024}; 16-byte aligned rows)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (((uintptr_t)dY | (uintptr_t)Y | (uintptr_t)G | (uintptr_t)workspace) & 15) { g_last_error = "gsr_relu_backward_bias: buffers must be 16-byte aligned"; return GSR_ERR_INVALID_ARGUMENT; }
    const int bands = (rows + RELU_BAND - 1) / RELU_BAND;
    if (bands > 0) hipLaunchKernelGGL(relu_bwd_bias_kernel, dim3((unsigned)bands), dim3(256), 0, stream, rows, cols, dY, Y, G, reinterpret_cast<float*>(workspace));
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)((cols + 15) / 16)), dim3(256), 0, stream, bands, cols, reinterpret_cast<const float*>(workspace), dbias);
    const int debug = 0;
    GSR_STAGE("gsr_relu_backward_bias");
    return 0;
}

int gsr_multi_add(int count, const gsr_multi_add_item* items, void* stream_)
{
    if (count < 0 || count > MULTI_ADD_MAX || (count > 0 && !items)) { g_last_error = "gsr_multi_add: 0 <= count <= 64 items"; return GSR_ERR_INVALID_ARGUMENT; }
    if (count == 0) return 0;
    MultiAddItems a;
    int largest = 0;
    for (int i = 0; i < count; i++) {
        const gsr_multi_add_item& q = items[i];
        if (q.count < 0 || (q.count > 0 && !q.dst)) { g_last_error = "gsr_multi_add: invalid item"; return GSR_ERR_INVALID_ARGUMENT; }
        a.item[i].dst = q.dst; a.item[i].count = q.count;
        for (int s = 0; s < MULTI_ADD_SOURCES; s++) a.item[i].src[s] = q.src[s];
        largest = std::max(largest, q.count);
    }
    if (largest == 0) return 0;
    hipLaunchKernelGGL(multi_add_kernel, dim3((unsigned)std::min((largest + 255) / 256, 64), (unsigned)count), dim3(256), 0, (hipStream_t)stream_, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_segment_sum(int B, int S, int E, int C, int Nv, const float* g, const char* csr_workspace, const int* set_of_b, float* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (B < 0 || S < 1 || E < 0 || C < 1 || Nv < 1 || !csr_workspace || (B > 0 && (!out || (E > 0 && !g)))) { g_last_error = "gsr_segment_sum: invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (B == 0) return 0;
    const IndexCsrWs w = index_csr_layout(S, E, Nv, csr_workspace);
    const size_t total = (size_t)B * Nv * C * SEG_LANES;
    hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, B, E, C, Nv, g, (size_t)E * C, (const int*)w.order, (const int*)w.seg,
                       set_of_b, out, (size_t)Nv * C);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_node_blend_backward(const gsr_node_blend* a, const float* nn_weight, const float* nn_dist, const int64_t* nn_idx,
                            const float* g_xyz, const float* g_rotation, const float* g_scaling, const float* g_nn_weight,
                            float* g_node_trans, float* g_node_rot, float* g_node_scale, float* g_node_frame, float* g_node_radius,
                            float* g_node_weight, char* workspace, void* stream_)
{
    return gsr_node_blend_backward_batch(a, 1, nn_weight, nn_dist, nn_idx, g_xyz, g_rotation, g_scaling, g_nn_weight, g_node_trans, g_node_rot, g_node_scale,
                                         g_node_frame, g_node_radius, g_node_weight, workspace, stream_);
}

int gsr_node_blend_backward_batch(const gsr_node_blend* a, int B, const float* nn_weight, const float* nn_dist, const int64_t* nn_idx,
                                  const float* g_xyz, const float* g_rotation, const float* g_scaling, const float* g_nn_weight,
                                  float* g_node_trans, float* g_node_rot, float* g_node_scale, float* g_node_frame, float* g_node_radius,
                                  float* g_node_weight, char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = node_blend_check(a, "gsr_node_blend_backward")) return rc;
    if (B < 1 || B > 65535 || (B > 1 && (g_nn_weight || !a->node_trans))) {
        g_last_error = "gsr_node_blend_backward_batch: 1 <= B <= 65535; B > 1 needs node attributes and takes no direct cotangent of nn_weight"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || (a->n > 0 && (!nn_weight || !nn_dist || !nn_idx))) { g_last_error = "gsr_node_blend_backward: null workspace / saved tensors"; return GSR_ERR_INVALID_ARGUMENT; }
    const NodeBlendWs ws = node_blend_layout(a->n, a->m, B, workspace);
    float* const partial = ws.partial;
    const int total = a->m * NODE_GRAD;
    const bool use_lds = a->m <= NODE_LDS_MAX;
    const size_t stride = ws.stride;
    // K <= 4 (every shipped call): the ordered route -- contributions written per (Gaussian, k), summed per node in the order of the Gaussians
    // (index_csr_kernel + segment_sum_kernel above): bit-reproducible. K > 4: round 3's LDS-atomic accumulation.
    const bool ordered = a->K <= NODE_DET_MAX_K && a->n > 0;
    float* summed;
    if (ordered) {
        const int E = (int)(a->n * a->K);
        float* contrib = partial;                                  // [B][E][21], batch stride `stride`
        summed = partial + (size_t)E * NODE_GRAD;
        hipLaunchKernelGGL(node_blend_bwd_kernel, dim3((unsigned)node_bwd_blocks(a->n), (unsigned)B), dim3(NODE_BLOCK), 0, stream, *a, nn_weight,
                           nn_dist, nn_idx, g_xyz, g_rotation, g_scaling, g_nn_weight, partial, 0, stride, contrib, stride);
        if (int rc = gsr_index_csr(1, E, a->m, nn_idx, ws.csr, stream_)) return rc;
        const IndexCsrWs csr = index_csr_layout(1, E, a->m, ws.csr);
        const size_t nthreads = (size_t)B * a->m * NODE_GRAD * SEG_LANES;
        hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream, B, E, NODE_GRAD, a->m, (const float*)contrib, stride,
                           (const int*)csr.order, (const int*)csr.seg, (const int*)nullptr, summed, stride);
    } else {
        const int G = use_lds ? node_bwd_blocks(a->n) : 1;
        if (!use_lds || a->n == 0) {
            for (int b = 0; b < B; b++) GSR_HIP_CHECK(hipMemsetAsync(partial + (size_t)b * stride, 0, (size_t)total * sizeof(float), stream));
        }
        if (a->n > 0) {
            const int blocks = node_bwd_blocks(a->n);
            hipLaunchKernelGGL(node_blend_bwd_kernel, dim3(blocks, (unsigned)B), dim3(NODE_BLOCK), use_lds ? (size_t)total * sizeof(float) : 0, stream, *a, nn_weight,
                               nn_dist, nn_idx, g_xyz, g_rotation, g_scaling, g_nn_weight, partial, use_lds ? 1 : 0, stride, (float*)nullptr, (size_t)0);
        }
        summed = partial + (size_t)G * total;
        hipLaunchKernelGGL(node_grad_reduce_kernel, dim3((total + 255) / 256, (unsigned)B), dim3(256), 0, stream, G, total, (const float*)partial, summed, stride);
    }
    hipLaunchKernelGGL(node_grad_finalize_kernel, dim3((a->m + 255) / 256, (unsigned)B), dim3(256), 0, stream, *a, (const float*)summed, g_node_trans, g_node_rot,
                       g_node_scale, g_node_frame, g_node_radius, g_node_weight, stride);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- map maintenance + camera step (include/slam_map.h) -----------------------------------------------------------------------
extern "C" {

// workspace of gsr_seed_from_rgbd: the mean squared distances [n] | gsr_knn_mean_dist2's workspace
struct SeedWs { float* dist2; char* knn; size_t bytes; };
static SeedWs seed_layout(int n, const char* workspace)
{
    Carver c(workspace, 256, true);
    return {c.take<float>((size_t)(n > 0 ? n : 1)), c.nested(gsr_knn_workspace_size(n)), c.bytes()};
}
size_t gsr_seed_workspace_size(int n) { return seed_layout(n, nullptr).bytes; }

int gsr_seed_from_rgbd(int n, const int* pix, int width, int height, const float* depth, const float* image, const float* exposure_a,
                       const float* exposure_b, float fx, float fy, float cx, float cy, const float* R, const float* T, float point_size,
                       int scale_dim, float* xyz, float* features_dc, float* log_scales, float* rotations, float* logit_opacity,
                       char* workspace, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || width <= 0 || height <= 0 || (scale_dim != 1 && scale_dim != 3) || !(fx != 0.f) || !(fy != 0.f)) {
        g_last_error = "gsr_seed_from_rgbd: invalid size / intrinsics / scale_dim"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return 0;
    if (!pix || !depth || !image || !R || !T || !xyz || !features_dc || !log_scales || !rotations || !logit_opacity || !workspace) {
        g_last_error = "gsr_seed_from_rgbd: null argument"; return GSR_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(seed_backproject_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, pix, width, height, depth, image, exposure_a,
                       exposure_b, fx, fy, cx, cy, R, T, xyz, features_dc, rotations, logit_opacity);
    const SeedWs w = seed_layout(n, workspace);
    if (int rc = gsr_knn_mean_dist2(n, xyz, w.dist2, w.knn, stream_)) return rc;
    hipLaunchKernelGGL(seed_scales_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, (const float*)w.dist2, point_size, scale_dim, log_scales);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_densify_select(int P, const float* xyz_gradient_accum, const float* denom, const float* log_scales, int scale_dim,
                       const float* logit_opacity, float grad_threshold, float dense_scale, float min_opacity, float big_scale, int* flags,
                       void* stream_)
{
    if (P < 0 || (scale_dim != 1 && scale_dim != 3)) { g_last_error = "gsr_densify_select: invalid size / scale_dim"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P == 0) return 0;
    if (!xyz_gradient_accum || !denom || !log_scales || !logit_opacity || !flags) { g_last_error = "gsr_densify_select: null argument"; return GSR_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(densify_select_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, P, xyz_gradient_accum, denom, log_scales,
                       scale_dim, logit_opacity, grad_threshold, dense_scale, min_opacity, big_scale, flags);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_densify_apply(int P, const int* flags, const int* offsets, int n_keep, int n_clone, int n_split, int n_child, int ntensors,
                      const gsr_densify_tensor* tensors, const float* xyz, const float* log_scales, int scale_dim, const float* raw_rotations,
                      const float* noise, void* stream_)
{
    if (P < 0 || n_keep < 0 || n_clone < 0 || n_split < 0 || n_child < 0 || ntensors < 0 || ntensors > DENSIFY_MAX_TENSORS || (ntensors > 0 && !tensors)) {
        g_last_error = "gsr_densify_apply: invalid counts (at most 32 tensors)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0 || ntensors == 0) return 0;
    if (!flags || !offsets) { g_last_error = "gsr_densify_apply: null flags / offsets"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n_child > 0 && (!xyz || !log_scales || !raw_rotations || !noise || (scale_dim != 1 && scale_dim != 3))) {
        g_last_error = "gsr_densify_apply: children need xyz, log_scales, raw_rotations and noise"; return GSR_ERR_INVALID_ARGUMENT;
    }
    DensifyArgs a;
    a.P = P; a.n_keep = n_keep; a.n_clone = n_clone; a.n_split = n_split; a.n_child = n_child; a.ntensors = ntensors; a.scale_dim = scale_dim;
    a.flags = flags; a.offsets = offsets; a.xyz = xyz; a.log_scales = log_scales; a.raw_rot = raw_rotations; a.noise = noise;
    const long long n_out = (long long)n_keep + n_clone + 2LL * n_child;
    for (int k = 0; k < ntensors; k++) {
        const gsr_densify_tensor& t = tensors[k];
        if (t.width <= 0 || !t.src || (n_out > 0 && !t.dst) || t.kind < GSR_DENSIFY_COPY || t.kind > GSR_DENSIFY_SCALE ||
            (t.kind == GSR_DENSIFY_XYZ && t.width != 3)) {
            g_last_error = "gsr_densify_apply: bad tensor descriptor"; return GSR_ERR_INVALID_ARGUMENT;
        }
        a.t[k] = DensifyTensor{t.src, t.dst, t.width, t.kind};
    }
    hipLaunchKernelGGL(densify_apply_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static int camera_step_args(const gsr_camera_step* s, CameraStepArgs& a)
{
    if (!s || !s->R || !s->T || !s->viewmatrix || (s->full_proj && !s->projmatrix)) { g_last_error = "gsr_camera_step_launch: null pose / output"; return GSR_ERR_INVALID_ARGUMENT; }
    const bool any_grad = s->g_rot_delta || s->g_trans_delta || s->g_exposure_a || s->g_exposure_b;
    if (any_grad && (!s->exp_avg || !s->exp_avg_sq || !s->step)) { g_last_error = "gsr_camera_step_launch: Adam state missing"; return GSR_ERR_INVALID_ARGUMENT; }
    if ((s->g_rot_delta && !s->rot_delta) || (s->g_trans_delta && !s->trans_delta) || (s->g_exposure_a && !s->exposure_a) || (s->g_exposure_b && !s->exposure_b) ||
        (s->do_pose && (!s->rot_delta || !s->trans_delta))) {
        g_last_error = "gsr_camera_step_launch: gradient / pose step without its parameter"; return GSR_ERR_INVALID_ARGUMENT;
    }
    a.p[0] = s->rot_delta; a.g[0] = s->g_rot_delta; a.n[0] = 3; a.lr[0] = s->lr_rot;
    a.p[1] = s->trans_delta; a.g[1] = s->g_trans_delta; a.n[1] = 3; a.lr[1] = s->lr_trans;
    a.p[2] = s->exposure_a; a.g[2] = s->g_exposure_a; a.n[2] = 1; a.lr[2] = s->lr_exposure;
    a.p[3] = s->exposure_b; a.g[3] = s->g_exposure_b; a.n[3] = 1; a.lr[3] = s->lr_exposure;
    a.exp_avg = s->exp_avg; a.exp_avg_sq = s->exp_avg_sq; a.step = s->step; a.beta1 = s->beta1; a.beta2 = s->beta2; a.eps = s->eps;
    a.R = s->R; a.T = s->T; a.proj = s->projmatrix; a.view = s->viewmatrix; a.full = s->full_proj; a.campos = s->campos;
    a.converged = s->converged; a.thr = s->converged_threshold; a.do_pose = s->do_pose; a.latch = s->latch;
    return 0;
}

int gsr_camera_step_launch(const gsr_camera_step* s, void* stream_)
{
    CameraStepArgs a;
    { const int rc = camera_step_args(s, a); if (rc) return rc; }
    hipLaunchKernelGGL(camera_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_track_step, packed floats (include/slam_map.h): dL/dimage [3, N] | dL/ddepth [N] | the exposure gradient's partials [T, 2] |
// the pose gradient {trans, rot} [6] | the exposure gradient [2]
struct TrackWs { float *g_image, *g_depth, *partials, *tau6, *g_exp; size_t bytes; };
static TrackWs track_layout(int width, int height, const char* workspace)
{
    const size_t N = (size_t)width * height, T = (size_t)((width + TILE_X - 1) / TILE_X) * ((height + TILE_Y - 1) / TILE_Y);
    Carver c(workspace, sizeof(float));
    return {c.take<float>(3 * N), c.take<float>(N), c.take<float>(2 * T), c.take<float>(6), c.take<float>(2), c.bytes()};
}
size_t gsr_track_workspace_size(int width, int height) { return width > 0 && height > 0 ? track_layout(width, height, nullptr).bytes : 0; }

int gsr_track_step(gsr_alloc_fn geometry_alloc, void* geometry_user, gsr_alloc_fn binning_alloc, void* binning_user, gsr_alloc_fn image_alloc,
                   void* image_user, int P, int D, int M, const float* background, int width, int height, const gsr_raw_inputs* in,
                   float scale_modifier, const float* projmatrix_raw, float tan_fovx, float tan_fovy, float* out_color, float* out_depth,
                   float* out_opacity, int* radii, int* n_touched, const gsr_track_loss* loss, const gsr_camera_step* step, float* dL_dmean2D,
                   char* workspace, void* stream)
{
    if (!in || !loss || !step || !workspace || !dL_dmean2D || !projmatrix_raw || P <= 0 || width <= 0 || height <= 0 || !loss->gt_image || !loss->gt_depth ||
        !step->full_proj || !step->campos || !step->rot_delta || !step->trans_delta || (step->exposure_a == nullptr) != (step->exposure_b == nullptr) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        g_last_error = "gsr_track_step: null / invalid argument (P > 0; loss targets, pose deltas, full_proj, campos, a 16-byte aligned workspace of gsr_track_workspace_size bytes)";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t N = (size_t)width * height;
    const auto [g_image, g_depth, partials, tau6, g_exp, ws_bytes] = track_layout(width, height, workspace);
    gsr_camera_step st = *step;                   // which tensors are stepped: the pose always, the exposure pair when it is given
    st.g_rot_delta = tau6 + 3; st.g_trans_delta = tau6;
    st.g_exposure_a = st.exposure_a ? g_exp : nullptr; st.g_exposure_b = st.exposure_b ? g_exp + 1 : nullptr;
    TrackTail tail;
    { const int rc = camera_step_args(&st, tail.step); if (rc) return rc; }
    tail.exposure_partials = partials; tail.dL_dexposure = g_exp;
    TrackLossArgs tl;
    tl.gt_image = loss->gt_image; tl.gt_depth = loss->gt_depth; tl.w_rgb = loss->w_rgb; tl.w_depth = loss->w_depth;
    tl.exposure_a = step->exposure_a; tl.exposure_b = step->exposure_b;
    tl.opacity_thr = loss->opacity_depth_threshold; tl.use_opacity = loss->opacity_weights ? 1 : 0;
    tl.c_rgb = loss->alpha / (3.0f * (float)N); tl.c_depth = (1.0f - loss->alpha) / (float)N;          // (make_loss_args)
    tl.dL_dimage = g_image; tl.dL_ddepth = g_depth; tl.partials = partials;
    Call c{read_options(), &spec_state(0)};
    c.track_loss = &tl;
    c.track_tail = &tail;
    FwdInputs fin;
    fin.raw = in;
    CapturedAllocs al{{geometry_alloc, geometry_user, nullptr}, {binning_alloc, binning_user, nullptr}, {image_alloc, image_user, nullptr}};
    const int R = forward_impl(c, al.fns(), P, D, M, background, width, height, fin, scale_modifier, {step->viewmatrix, step->full_proj, step->campos, tan_fovx, tan_fovy},
                               {out_color, out_depth, out_opacity, radii, n_touched}, 0, stream);
    if (R < 0) return R;
    const gsr_raw_grads none{};
    BwdGrads g;
    g.dL_dmean2D = dL_dmean2D; g.dL_dtau_sum = tau6;
    const int rc = backward_impl(c, P, D, M, background, width, height, fin, scale_modifier, {step->viewmatrix, step->full_proj, step->campos, tan_fovx, tan_fovy, projmatrix_raw},
                                 {al.g.got, al.b.got, al.i.got, radii, R}, {g_image, g_depth}, g, &none, GSR_BACKWARD_POSE_ONLY, stream);
    if (rc < 0) return rc;
    GSR_HIP_CHECK(hipGetLastError());
    return R;
}

int gsr_camera_steps_launch(int n, const gsr_camera_step* steps, void* stream_)
{
    if (n < 0 || n > CAMERA_STEPS_MAX || (n > 0 && !steps)) { g_last_error = "gsr_camera_steps_launch: 0..12 cameras"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n == 0) return 0;
    CameraStepsArgs all;
    memset(&all, 0, sizeof(all));
    for (int k = 0; k < n; k++) { const int rc = camera_step_args(&steps[k], all.c[k]); if (rc) return rc; }
    hipLaunchKernelGGL(camera_steps_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream_, all);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_schedule_advance(int* counter, const unsigned int* table, int row_words, int rows, unsigned int* current, void* stream_)
{
    if (!counter || !table || !current || row_words < 1 || rows < 1) { g_last_error = "gsr_schedule_advance: null / empty argument"; return GSR_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, counter, (const uint32_t*)table, row_words, rows, (uint32_t*)current);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_slot_gather(int n_slots, const gsr_keyframe_entry* table, const int* index, const gsr_keyframe_entry* dst, int pixels, void* stream_)
{
    if (n_slots < 0 || n_slots > SLOTS_MAX || pixels < 1 || (n_slots > 0 && (!table || !index || !dst))) {
        g_last_error = "gsr_slot_gather: 0..4 slots, device table / index and a host array of destinations"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n_slots == 0) return 0;
    static_assert(sizeof(gsr_keyframe_entry) == sizeof(KeyframeEntry), "gsr_keyframe_entry layout");
    SlotGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.n_slots = n_slots; a.pixels = pixels; a.table = reinterpret_cast<const KeyframeEntry*>(table); a.index = index;
    for (int s = 0; s < n_slots; s++) {
        if (!dst[s].viewmatrix || !dst[s].full_proj || !dst[s].campos) { g_last_error = "gsr_slot_gather: a slot needs viewmatrix / full_proj / campos buffers"; return GSR_ERR_INVALID_ARGUMENT; }
        memcpy(&a.dst[s], &dst[s], sizeof(KeyframeEntry));
    }
    hipLaunchKernelGGL(slot_gather_kernel, dim3(SLOT_GATHER_BLOCKS, (unsigned)n_slots), dim3(256), 0, (hipStream_t)stream_, a);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_edge_mask(const float* image, int height, int width, float edge_threshold, float eps, float* intensity, float* median,
                  unsigned char* mask, void* stream_)
{
    if (!image || !intensity || !median || !mask || height < 2 || width < 2) { g_last_error = "gsr_edge_mask: null argument or image smaller than 2x2"; return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = (hipStream_t)stream_;
    const int n = height * width;
    hipLaunchKernelGGL(edge_intensity_kernel, dim3((width + 15) / 16, (height + 15) / 16), dim3(256), 0, stream, image, height, width, eps, intensity);
    // scratch of the radix select (260 words per device, allocated once; the selects of one device are stream-ordered by their callers)
    static uint32_t* select_state[16] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (!select_state[dev]) GSR_HIP_CHECK(hipMalloc((void**)&select_state[dev], 260 * sizeof(uint32_t)));
    GSR_HIP_CHECK(hipMemsetAsync(select_state[dev], 0, 260 * sizeof(uint32_t), stream));
    for (int shift = 24; shift >= 0; shift -= 8)      // torch.median: the lower one of the two middle elements
        hipLaunchKernelGGL(radix_select_pass_kernel, dim3(SELECT_BLOCKS), dim3(1024), 0, stream, (const float*)intensity, n, (n - 1) / 2, shift, select_state[dev], median);
    hipLaunchKernelGGL(edge_compare_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const float*)intensity, n, (const float*)median, edge_threshold, mask);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_mono_keyframe_depth (the byte offsets: gs_map.h): the select's state, 260 words | {n_valid, the select's output} |
// 64 x {s1, s2} doubles | the keys [n]
struct MonoWs { uint32_t* state; uint32_t* n_valid; float* median; double* partial; uint32_t* keys; size_t bytes; };
static MonoWs mono_layout(int height, int width, const char* workspace)
{
    Carver c(workspace, 16);
    uint32_t* const state = c.take<uint32_t>(260), * const n_valid = c.take<uint32_t>(2);
    return {state, n_valid, reinterpret_cast<float*>(n_valid ? n_valid + 1 : nullptr), c.take<double>(2 * SELECT_BLOCKS),
            c.take<uint32_t>(height > 0 && width > 0 ? (size_t)height * (size_t)width : 0), c.bytes()};
}
size_t gsr_mono_keyframe_depth_workspace_size(int height, int width) { return mono_layout(height, width, nullptr).bytes; }

int gsr_mono_keyframe_depth(const float* depth, const float* opacity, const float* gt_image, int height, int width, float rgb_boundary_threshold,
                            const float* noise, float* out, float* stats, char* workspace, void* stream_)
{
    if (!depth || !opacity || !gt_image || !noise || !out || !stats || !workspace || height < 1 || width < 1 || (long long)height * width > (1ll << 28)) {
        g_last_error = "gsr_mono_keyframe_depth: null argument or an image of less than 1 or more than 2^28 pixels"; return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) { g_last_error = "gsr_mono_keyframe_depth: the workspace must be 16-byte aligned"; return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = (hipStream_t)stream_;
    const int n = height * width;
    const auto [state, n_valid, median, partial, keys, ws_bytes] = mono_layout(height, width, workspace);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    GSR_HIP_CHECK(hipMemsetAsync(workspace, 0, reinterpret_cast<char*>(partial) - workspace, stream));   // select state, n_valid, the select's output
    hipLaunchKernelGGL(mono_keys_kernel, dim3(blocks), dim3(256), 0, stream, depth, opacity, gt_image, n, rgb_boundary_threshold, keys, n_valid);
    for (int shift = 24; shift >= 0; shift -= 8)
        hipLaunchKernelGGL(radix_select_counted_pass_kernel, dim3(SELECT_BLOCKS), dim3(1024), 0, stream, reinterpret_cast<const float*>(keys), n,
                           (const uint32_t*)n_valid, shift, state, median);
    hipLaunchKernelGGL(mono_moments_kernel, dim3(SELECT_BLOCKS), dim3(1024), 0, stream, (const uint32_t*)keys, n, (const uint32_t*)n_valid, (const float*)median, partial);
    hipLaunchKernelGGL(mono_depth_kernel, dim3(blocks), dim3(256), 0, stream, depth, opacity, gt_image, noise, n, rgb_boundary_threshold,
                       (const uint32_t*)n_valid, (const float*)median, (const double*)partial, out, stats);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t gsr_isotropic_loss_workspace_size(int P) { return P > 0 ? (size_t)((P + 255) / 256) * sizeof(float) + 16 : 16; }

int gsr_isotropic_loss_forward(int P, const float* raw_scales, float* loss, char* workspace, void* stream_)
{
    if (P < 0 || !loss || !workspace || (P > 0 && !raw_scales)) { g_last_error = "gsr_isotropic_loss_forward: invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    const int nb = (P + 255) / 256;
    float* partial = reinterpret_cast<float*>(workspace);
    if (nb) hipLaunchKernelGGL(isotropic_partial_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream_, P, raw_scales, partial);
    hipLaunchKernelGGL(isotropic_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, nb, P, (const float*)partial, loss);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_isotropic_loss_backward(int P, const float* raw_scales, const float* g_loss, float* d_raw_scales, void* stream_)
{
    if (P < 0 || (P > 0 && (!raw_scales || !g_loss || !d_raw_scales))) { g_last_error = "gsr_isotropic_loss_backward: invalid argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (P) hipLaunchKernelGGL(isotropic_backward_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, P, raw_scales, g_loss, d_raw_scales);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_arap_forward(int V, int T, int M, int K, const float* p, const float* nb, const float* keep, float* R, float* partial, void* stream_)
{
    if (V < 0 || T < 2 || M < 0 || K < 1 || ((size_t)V * M > 0 && (!p || !nb || !keep || !R || !partial))) {
        g_last_error = "gsr_arap_forward: invalid argument (T >= 2, K >= 1, no null buffers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t n = (size_t)V * (T - 1) * M;
    if (n > 0x7fffffffull) { g_last_error = "gsr_arap_forward: too many (view, sample, node) triples"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n) hipLaunchKernelGGL(arap_forward_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, V, T, M, K, p, nb, keep, R, partial);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_arap_backward(int V, int T, int M, int K, const float* p, const float* nb, const float* keep, const float* R, const float* g_partial,
                      float* dp, float* dnb, void* stream_)
{
    if (V < 0 || T < 2 || M < 0 || K < 1 || ((size_t)V * M > 0 && (!p || !nb || !keep || !R || !g_partial || !dp || !dnb))) {
        g_last_error = "gsr_arap_backward: invalid argument (T >= 2, K >= 1, no null buffers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t n = (size_t)V * M;
    if (n) hipLaunchKernelGGL(arap_backward_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, V, T, M, K, p, nb, keep, R, g_partial, dp, dnb);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_elastic_forward(int V, int M, int K, int T, const float* x, const float* nb, float* ratio, void* stream_)
{
    if (V < 0 || M < 0 || K < 1 || T < 2 || T > ELASTIC_MAX_T || ((size_t)V * M > 0 && (!x || !nb || !ratio))) {
        g_last_error = "gsr_elastic_forward: invalid argument (2 <= T <= 16, K >= 1, no null buffers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t n = (size_t)V * M * K;
    if (n) hipLaunchKernelGGL(elastic_forward_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, (int)n, M, K, T, x, nb, ratio);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_elastic_backward(int V, int M, int K, int T, const float* x, const float* nb, const float* g_ratio, float* dx, float* dnb, void* stream_)
{
    if (V < 0 || M < 0 || K < 1 || T < 2 || T > ELASTIC_MAX_T || ((size_t)V * M > 0 && (!x || !nb || !g_ratio || !dx || !dnb))) {
        g_last_error = "gsr_elastic_backward: invalid argument (2 <= T <= 16, K >= 1, no null buffers)"; return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t n = (size_t)V * M * K, nx = (size_t)V * M * T * 3;
    if (n) {
        hipLaunchKernelGGL(elastic_backward_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, (int)n, M, K, T, x, nb, g_ratio, dnb);
        hipLaunchKernelGGL(elastic_backward_self_kernel, dim3((unsigned)((nx + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, (int)nx, K, T * 3, dnb, dx);
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_kabsch_rotations(int n, const float* S, float* R, void* stream_)
{
    if (n < 0 || (n > 0 && (!S || !R))) { g_last_error = "gsr_kabsch_rotations: null argument"; return GSR_ERR_INVALID_ARGUMENT; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(kabsch_rotation_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream_, n, S, R);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_frame_prepare(int width, int height, const unsigned char* rgb, const float* map_xy, const float* lut, const unsigned char* mask_l,
                      float mask_threshold, float* image, unsigned char* motion, void* stream_)
{
    if (!rgb || !lut || !image) { g_last_error = "gsr_frame_prepare: rgb, lut and image must not be NULL"; return GSR_ERR_INVALID_ARGUMENT; }
    if (width <= 0 || height <= 0 || (long long)width * height * 3 > 0x7fffffffLL) {
        g_last_error = "gsr_frame_prepare: width and height must be positive and width * height * 3 below 2^31";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (mask_l && !motion) { g_last_error = "gsr_frame_prepare: mask_l given without a motion output"; return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = (hipStream_t)stream_;
    const int n = width * height;
    ScopedKernelTimer tm(K_FRAME_PREPARE, stream);
    hipLaunchKernelGGL(frame_prepare_kernel, dim3((unsigned)((n + FRAME_BLOCK - 1) / FRAME_BLOCK)), dim3(FRAME_BLOCK), 0, stream, width, height, rgb,
                       reinterpret_cast<const float2*>(map_xy), lut, mask_l, mask_threshold, image, motion);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_frame_export(int views, int width, int height, const float* colour, int64_t colour_stride, const float* depth, int64_t depth_stride,
                     const unsigned char* lut, float depth_vmax, float depth_scale, unsigned char* rgb8, unsigned char* depth_rgb8,
                     unsigned short* depth_u16, void* stream_)
{
    if (!colour || !lut || !rgb8) { g_last_error = "gsr_frame_export: colour, lut and rgb8 must not be NULL"; return GSR_ERR_INVALID_ARGUMENT; }
    if ((depth_rgb8 || depth_u16) && !depth) { g_last_error = "gsr_frame_export: a depth output was asked for without depth"; return GSR_ERR_INVALID_ARGUMENT; }
    if (views <= 0 || views > 65535 || width <= 0 || height <= 0 || (long long)width * height * 3 > 0x7fffffffLL) {
        g_last_error = "gsr_frame_export: views must be in [1, 65535], width and height positive and width * height * 3 below 2^31";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const long long n = (long long)width * height;
    if (colour_stride < 3 * n || (depth && depth_stride < n)) {
        g_last_error = "gsr_frame_export: a view stride is smaller than the view (3 * width * height floats of colour, width * height of depth)";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(depth_vmax > 0.0f)) { g_last_error = "gsr_frame_export: depth_vmax must be positive"; return GSR_ERR_INVALID_ARGUMENT; }
    if (((size_t)rgb8 | (size_t)depth_rgb8) & 3 || ((size_t)depth_u16 & 7)) {
        g_last_error = "gsr_frame_export: rgb8 and depth_rgb8 must be 4-byte aligned, depth_u16 8-byte aligned";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const long long threads = (long long)((width + 3) / 4) * height;
    hipLaunchKernelGGL(frame_export_kernel, dim3((unsigned)((threads + FRAME_BLOCK - 1) / FRAME_BLOCK), (unsigned)views), dim3(FRAME_BLOCK), 0, stream,
                       width, height, colour, colour_stride, depth, depth_stride, lut, depth_vmax, depth_scale, rgb8, depth_rgb8, depth_u16);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_jpeg_encode: coefficients [V, blocks, 64] int16 | bit lengths, then offsets [V, blocks] u32 | total bits [V] u32 | the bit
// buffers [V, raw_words] u32; every part starts on a multiple of 16 bytes
struct JpegLayout { JpegShape shape; short* coef; uint32_t *lengths, *totals, *raw; size_t bytes; };
static bool jpeg_layout(int views, int width, int height, const void* workspace, JpegLayout& l)
{
    if (views <= 0 || views > 65535 || width <= 0 || height <= 0 || width > 65535 || height > 65535) return false;
    const long long cols = (width + 15) / 16, rows = (height + 15) / 16, blocks = cols * rows * 6;
    if (blocks > 1290000) return false;                              // blocks * 1664 bits stay below 2^31
    l.shape.W = width; l.shape.H = height; l.shape.mcu_cols = (int)cols; l.shape.blocks = (int)blocks;
    l.shape.raw_words = (size_t)blocks * JPEG_BLOCK_WORDS + JPEG_TAIL_WORDS;
    Carver c(workspace, 16);
    l.coef = c.take<short>((size_t)views * blocks * 64);
    l.lengths = c.take<uint32_t>((size_t)views * blocks);
    l.totals = c.take<uint32_t>((size_t)views);
    l.raw = c.take<uint32_t>((size_t)views * l.shape.raw_words);
    l.bytes = c.bytes();
    return true;
}

size_t gsr_jpeg_workspace_size(int views, int width, int height) { JpegLayout l; return jpeg_layout(views, width, height, nullptr, l) ? l.bytes : 0; }

int gsr_jpeg_encode(int views, int width, int height, const unsigned char* rgb8, const unsigned short* qtables, unsigned char* scan,
                    int64_t scan_stride, int* sizes, short* coefficients, void* workspace, size_t workspace_bytes, void* stream_)
{
    JpegLayout l;
    if (!jpeg_layout(views, width, height, workspace, l)) {
        g_last_error = "gsr_jpeg_encode: views, width and height must be in [1, 65535], with at most 1290000 8x8 blocks per view";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!rgb8 || !qtables || !scan || !sizes || !workspace) {
        g_last_error = "gsr_jpeg_encode: rgb8, qtables, scan, sizes and workspace must not be NULL";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (scan_stride <= 0) { g_last_error = "gsr_jpeg_encode: scan_stride must be positive"; return GSR_ERR_INVALID_ARGUMENT; }
    if (!workspace_fits("gsr_jpeg_encode", "gsr_jpeg_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    short* const coef = l.coef;
    uint32_t* const lengths = l.lengths, * const totals = l.totals, * const raw = l.raw;
    const dim3 per_block((unsigned)((l.shape.blocks + JPEG_WAVES - 1) / JPEG_WAVES), (unsigned)views);
    hipLaunchKernelGGL(jpeg_transform_kernel, per_block, dim3(JPEG_BLOCK), 0, stream, l.shape, rgb8, qtables, coef, coefficients, lengths, raw);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((unsigned)views), dim3(JPEG_SCAN_BLOCK), 0, stream, l.shape, coef, lengths, totals);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_emit_kernel, per_block, dim3(JPEG_BLOCK), 0, stream, l.shape, coef, lengths, raw);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)views), dim3(JPEG_SCAN_BLOCK), 0, stream, l.shape, raw, totals, scan, (long long)scan_stride, sizes);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_jpeg_decode: coefficients [F, mcus, blocks per MCU, 64] int16 (unused when the caller takes them) | restart marker
// positions [F, max_intervals] i32 | markers found [F] i32 | the intervals' results [F, max_intervals] i32 | the component planes
// [F, Y | Cb | Cr] bytes; every part starts on a multiple of 16 bytes
struct JpegDecodeLayout { JpegDecodeShape shape; short* coef; int *marks, *mcount, *ivfail; unsigned char* planes; size_t bytes; };
static bool jpeg_decode_layout(int frames, int width, int height, int sampling, int max_intervals, const void* workspace, JpegDecodeLayout& l)
{
    if (frames <= 0 || frames > 65535 || width <= 0 || height <= 0 || width > 65535 || height > 65535) return false;
    if (sampling < GSR_JPEG_GREY || sampling > GSR_JPEG_420) return false;
    JpegDecodeShape& s = l.shape;
    s.frames = frames; s.W = width; s.H = height;
    s.hs = sampling >= GSR_JPEG_422 ? 2 : 1;
    s.vs = sampling == GSR_JPEG_420 ? 2 : 1;
    s.comps = sampling == GSR_JPEG_GREY ? 1 : 3;
    s.bpm = s.comps == 1 ? 1 : s.hs * s.vs + 2;
    const long long cols = (width + 8 * s.hs - 1) / (8 * s.hs), rows = (height + 8 * s.vs - 1) / (8 * s.vs), mcus = cols * rows;
    if (mcus * s.bpm > 1290000) return false;                        // the same ceiling as the encoder
    if (max_intervals < 1 || max_intervals > mcus) return false;
    s.mcu_cols = (int)cols; s.mcus = (int)mcus; s.cap = max_intervals;
    s.yW = (int)cols * 8 * s.hs; s.yH = (int)rows * 8 * s.vs;
    s.cW = s.comps == 1 ? 0 : (int)cols * 8; s.cH = s.comps == 1 ? 0 : (int)rows * 8;
    s.cw = (width + s.hs - 1) / s.hs; s.ch = (height + s.vs - 1) / s.vs;
    s.scan_bytes = 0;
    Carver c(workspace, 16);
    l.coef = c.take<short>((size_t)frames * mcus * s.bpm * 64);
    l.marks = c.take<int>((size_t)frames * max_intervals);
    l.mcount = c.take<int>((size_t)frames);
    l.ivfail = c.take<int>((size_t)frames * max_intervals);
    l.planes = c.take<unsigned char>((size_t)frames * ((size_t)s.yW * s.yH + 2 * (size_t)s.cW * s.cH));
    l.bytes = c.bytes();
    return true;
}

size_t gsr_jpeg_decode_workspace_size(int frames, int width, int height, int sampling, int max_intervals)
{
    JpegDecodeLayout l;
    return jpeg_decode_layout(frames, width, height, sampling, max_intervals, nullptr, l) ? l.bytes : 0;
}

int gsr_jpeg_decode(int frames, int width, int height, int sampling, int max_intervals, const unsigned char* scans, const int64_t* offsets,
                    int64_t scan_bytes, const unsigned short* qtables, const int* huffman, const int* descriptors, unsigned char* rgb8,
                    int* status, short* coefficients, void* workspace, size_t workspace_bytes, void* stream_)
{
    JpegDecodeLayout l;
    if (!jpeg_decode_layout(frames, width, height, sampling, max_intervals, workspace, l)) {
        g_last_error = "gsr_jpeg_decode: frames, width and height must be in [1, 65535] with at most 1290000 8x8 blocks per frame, sampling one of "
                       "GSR_JPEG_GREY .. GSR_JPEG_420, max_intervals in [1, MCUs per frame]";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!scans || !offsets || !qtables || !huffman || !descriptors || !rgb8 || !status || !workspace) {
        g_last_error = "gsr_jpeg_decode: scans, offsets, qtables, huffman, descriptors, rgb8, status and workspace must not be NULL";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (scan_bytes < 0) { g_last_error = "gsr_jpeg_decode: scan_bytes must not be negative"; return GSR_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<size_t>(coefficients) & 15) { g_last_error = "gsr_jpeg_decode: coefficients must be 16-byte aligned"; return GSR_ERR_INVALID_ARGUMENT; }
    if (!workspace_fits("gsr_jpeg_decode", "gsr_jpeg_decode_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    JpegDecodeShape s = l.shape;
    s.scan_bytes = scan_bytes;
    const long long* offs = reinterpret_cast<const long long*>(offsets);
    short* const coef = coefficients ? coefficients : l.coef;
    {
        ScopedKernelTimer tm(K_JPEGD_ENTROPY, stream);                // the serial part: restart markers and entropy decoding
        hipLaunchKernelGGL(jpegd_markers_kernel, dim3((unsigned)frames), dim3(JPEGD_BLOCK), 0, stream, s, scans, offs, l.marks, l.mcount);
        GSR_HIP_CHECK(hipGetLastError());
        const long long lanes = (long long)frames * max_intervals;
        hipLaunchKernelGGL(jpegd_entropy_kernel, dim3((unsigned)((lanes + JPEGD_ENTROPY_BLOCK - 1) / JPEGD_ENTROPY_BLOCK)), dim3(JPEGD_ENTROPY_BLOCK),
                           0, stream, s, scans, offs, huffman, descriptors, l.marks, l.mcount, coef, l.ivfail);
        GSR_HIP_CHECK(hipGetLastError());
    }
    ScopedKernelTimer tm(K_JPEGD_PIXELS, stream);                     // the parallel part: inverse DCT, upsampling and colour
    const int blocks = s.mcus * s.bpm;
    hipLaunchKernelGGL(jpegd_idct_kernel, dim3((unsigned)((blocks + JPEGD_BLOCK - 1) / JPEGD_BLOCK), (unsigned)frames), dim3(JPEGD_BLOCK), 0, stream,
                       s, coef, qtables, l.planes);
    GSR_HIP_CHECK(hipGetLastError());
    const long long pixels = (long long)width * height;
    hipLaunchKernelGGL(jpegd_colour_kernel, dim3((unsigned)((pixels + JPEGD_BLOCK - 1) / JPEGD_BLOCK), (unsigned)frames), dim3(JPEGD_BLOCK), 0, stream,
                       s, l.planes, descriptors, l.mcount, l.ivfail, rgb8, status);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_png_encode: the segments' staging slots [V, nseg, PNG_SLOT] bytes | their sizes [V, nseg] u32 | their Adler sums
// [V, nseg, 2] u32 | their offsets in the stream [V, nseg] u32; every part starts on a multiple of 16 bytes
struct PngLayout { PngShape shape; unsigned char* staging; uint32_t *seg_bytes, *seg_sums, *offsets; size_t bytes; long long bound; };
static bool png_layout(int views, int width, int height, int kind, const void* workspace, PngLayout& l)
{
    if (views <= 0 || views > 65535 || width <= 0 || height <= 0 || (kind != 0 && kind != 1)) return false;
    const long long D = kind == 0 ? 3 : 2, row = (long long)width * D + 1;
    if (row > 0x7fffffffLL / height) return false;
    const long long n = row * height, nseg = (n + PNG_SEG - 1) / PNG_SEG;
    l.bound = PNG_HEAD + n + PNG_SEG_EXTRA * nseg + PNG_TAIL;
    if (l.bound > 0x7fffffffLL) return false;                        // offsets and sizes are 32-bit
    l.shape.W = width; l.shape.H = height; l.shape.D = (int)D; l.shape.kind = kind; l.shape.filter = 0;
    l.shape.row = (int)row; l.shape.n = (int)n; l.shape.nseg = (int)nseg;
    const size_t segments = (size_t)views * (size_t)nseg;
    Carver c(workspace, 16);
    l.staging = c.take<unsigned char>(segments * PNG_SLOT);
    l.seg_bytes = c.take<uint32_t>(segments);
    l.seg_sums = c.take<uint32_t>(segments * 2);
    l.offsets = c.take<uint32_t>(segments);
    l.bytes = c.bytes();
    return true;
}

size_t gsr_png_workspace_size(int views, int width, int height, int kind)
{
    PngLayout l;
    return png_layout(views, width, height, kind, nullptr, l) ? l.bytes : 0;
}

size_t gsr_png_stream_bound(int width, int height, int kind)
{
    PngLayout l;
    return png_layout(1, width, height, kind, nullptr, l) ? (size_t)l.bound : 0;
}

int gsr_png_encode(int views, int width, int height, int kind, int filter, const void* pixels, unsigned char* out, int64_t out_stride, int* sizes,
                   void* workspace, size_t workspace_bytes, void* stream_)
{
    if (kind != 0 && kind != 1) { g_last_error = "gsr_png_encode: kind must be 0 (8-bit RGB) or 1 (16-bit grey)"; return GSR_ERR_INVALID_ARGUMENT; }
    if (filter != 0 && filter != 2) { g_last_error = "gsr_png_encode: filter must be 0 (None) or 2 (Up)"; return GSR_ERR_INVALID_ARGUMENT; }
    PngLayout l;
    if (!png_layout(views, width, height, kind, workspace, l)) {
        g_last_error = "gsr_png_encode: views must be in [1, 65535], width and height positive, and a view's stream bound (gsr_png_stream_bound) below 2^31";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const char* const null_name = !pixels ? "pixels" : !out ? "out" : !sizes ? "sizes" : !workspace ? "workspace" : nullptr;
    if (null_name) { g_last_error = std::string("gsr_png_encode: ") + null_name + " must not be NULL"; return GSR_ERR_INVALID_ARGUMENT; }
    if (out_stride < l.bound) {
        g_last_error = "gsr_png_encode: out_stride must be at least gsr_png_stream_bound = " + std::to_string(l.bound) + " bytes, got " + std::to_string(out_stride);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!workspace_fits("gsr_png_encode", "gsr_png_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    l.shape.filter = filter;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 per_segment((unsigned)l.shape.nseg, (unsigned)views);
    hipLaunchKernelGGL(png_segment_kernel, per_segment, dim3(PNG_BLOCK), 0, stream, l.shape, static_cast<const unsigned char*>(pixels), l.staging,
                       l.seg_bytes, l.seg_sums);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(png_offsets_kernel, dim3((unsigned)views), dim3(PNG_SCAN_BLOCK), 0, stream, l.shape, l.seg_bytes, l.seg_sums, l.offsets, out,
                       (long long)out_stride, sizes);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(png_gather_kernel, per_segment, dim3(PNG_BLOCK), 0, stream, l.shape, l.staging, l.seg_bytes, l.offsets, out, (long long)out_stride);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_stereo_depth: census codes of the left and of the right image [H, W] u64 | S [H, W, D] u16 (unused when the caller
// gives cost_sum); every part starts on a multiple of 16 bytes
struct StereoLayout { uint64_t *code_l, *code_r; unsigned short* cost; size_t bytes; };
static bool stereo_layout(int width, int height, int D, const void* workspace, StereoLayout& l)
{
    if (width < 1 || height < 1 || (D != 64 && D != 128) || (long long)width * height * D > 0x7fffffffLL) return false;
    const size_t n = (size_t)width * height;
    Carver c(workspace, 16);
    l.code_l = c.take<uint64_t>(n);
    l.code_r = c.take<uint64_t>(n);
    l.cost = c.take<unsigned short>(n * D);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_stereo_workspace_size(int width, int height, int D) { StereoLayout l; return stereo_layout(width, height, D, nullptr, l) ? l.bytes : 0; }

int gsr_stereo_depth(int width, int height, int num_disparities, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, float bf,
                     const unsigned char* left_raw, const unsigned char* right_raw, const float* map_left, const float* map_right,
                     const float* lut, unsigned char* left_rect, unsigned char* right_rect, float* image, short* disparity16, float* depth,
                     unsigned short* cost_sum, void* workspace, size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_stereo_depth: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    StereoLayout l;
    if (!stereo_layout(width, height, num_disparities, workspace, l))
        return fail("width and height must be positive, num_disparities 64 or 128 (got " + std::to_string(num_disparities) +
                    ") and width * height * num_disparities below 2^31");
    if (!(p1 > 0 && p1 < p2 && p2 <= 2047)) return fail("the penalties must satisfy 0 < p1 < p2 <= 2047, got p1 " + std::to_string(p1) + ", p2 " + std::to_string(p2));
    if (uniqueness_ratio < 0 || uniqueness_ratio > 99) return fail("uniqueness_ratio must be in [0, 99], got " + std::to_string(uniqueness_ratio));
    if (disp12_max_diff < -1) return fail("disp12_max_diff must be -1 (no check) or larger, got " + std::to_string(disp12_max_diff));
    if (!left_raw || !right_raw || !disparity16 || !workspace) return fail("left_raw, right_raw, disparity16 and workspace must not be NULL");
    if ((map_left != nullptr) != (map_right != nullptr)) return fail("map_left and map_right go together: both or neither");
    if (map_left && (!left_rect || !right_rect)) return fail("left_rect and right_rect must not be NULL when maps are given");
    if (image && !lut) return fail("image needs lut");
    if (!workspace_fits("gsr_stereo_depth", "gsr_stereo_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    if ((num_disparities == 128 && cost_sum && ((size_t)cost_sum & 3))) return fail("cost_sum must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    uint64_t* const code_l = l.code_l, * const code_r = l.code_r;
    unsigned short* S = cost_sum ? cost_sum : l.cost;
    const size_t n = (size_t)width * height;
    const unsigned pixel_blocks = (unsigned)((n + STEREO_BLOCK - 1) / STEREO_BLOCK);
    if (map_left || left_rect || right_rect || image) {
        hipLaunchKernelGGL(stereo_rectify_kernel, dim3(pixel_blocks, 2), dim3(STEREO_BLOCK), 0, stream, width, height, left_raw, right_raw,
                           reinterpret_cast<const float2*>(map_left), reinterpret_cast<const float2*>(map_right), lut, left_rect, right_rect, image);
        GSR_HIP_CHECK(hipGetLastError());
    }
    const unsigned char* img_l = map_left ? left_rect : left_raw;
    const unsigned char* img_r = map_left ? right_rect : right_raw;
    hipLaunchKernelGGL(stereo_census_kernel, dim3(pixel_blocks, 2), dim3(STEREO_BLOCK), 0, stream, width, height, img_l, img_r, code_l, code_r);
    GSR_HIP_CHECK(hipGetLastError());
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    for (int r = 0; r < 8; ++r) {
        const int dx = dirs[r][0], dy = dirs[r][1];
        const unsigned paths = (unsigned)(dy == 0 ? height : dx == 0 ? width : width + height - 1);
        if (num_disparities == 64)
            hipLaunchKernelGGL(stereo_path_kernel<1>, dim3(paths), dim3(64), 0, stream, width, height, dx, dy, p1, p2, code_l, code_r, S, (int)(r == 0));
        else
            hipLaunchKernelGGL(stereo_path_kernel<2>, dim3(paths), dim3(64), 0, stream, width, height, dx, dy, p1, p2, code_l, code_r, S, (int)(r == 0));
        GSR_HIP_CHECK(hipGetLastError());
    }
    const float bf16 = (float)((double)bf * 16.0);                       // formed in double, rounded once
    const unsigned select_blocks = (unsigned)((n + STEREO_BLOCK / 64 - 1) / (STEREO_BLOCK / 64));
    if (num_disparities == 64)
        hipLaunchKernelGGL(stereo_select_kernel<1>, dim3(select_blocks), dim3(STEREO_BLOCK), 0, stream, width, height, uniqueness_ratio, disp12_max_diff,
                           bf16, S, disparity16, depth);
    else
        hipLaunchKernelGGL(stereo_select_kernel<2>, dim3(select_blocks), dim3(STEREO_BLOCK), 0, stream, width, height, uniqueness_ratio, disp12_max_diff,
                           bf16, S, disparity16, depth);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_sweep_depth: census codes of the reference and of the partners [1 + J, H, W] u64 | C [H, W, 64] u8 (unused when the
// caller gives cost) | S [H, W, 64] u16 (unused when the caller gives cost_sum) | the observability flags [H, W] u8; every part starts on
// a multiple of 16 bytes
struct SweepLayout { uint64_t* codes; unsigned char* cost; unsigned short* cost_sum; unsigned char* observable; size_t bytes; };
static bool sweep_layout(int width, int height, int partners, const void* workspace, SweepLayout& l)
{
    if (width < 1 || height < 1 || partners < 1 || partners > SWEEP_MAX_PARTNERS || (long long)width * height * SWEEP_D > 0x7fffffffLL) return false;
    const size_t n = (size_t)width * height;
    Carver c(workspace, 16);
    l.codes = c.take<uint64_t>(n * (size_t)(1 + partners));
    l.cost = c.take<unsigned char>(n * SWEEP_D);
    l.cost_sum = c.take<unsigned short>(n * SWEEP_D);
    l.observable = c.take<unsigned char>(n);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_sweep_workspace_size(int width, int height, int partners) { SweepLayout l; return sweep_layout(width, height, partners, nullptr, l) ? l.bytes : 0; }

int gsr_sweep_depth(int width, int height, int partners, float fx, float fy, float cx, float cy, float w_min, float w_step, int p1, int p2,
                    int uniqueness_ratio, int min_span_px, const unsigned char* ref_grey, const unsigned char* partner_grey,
                    const float* transforms, short* index16, float* depth, unsigned char* cost, unsigned short* cost_sum, void* workspace,
                    size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_sweep_depth: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    SweepLayout l;
    if (!sweep_layout(width, height, partners, workspace, l))
        return fail("width and height must be positive, partners in [1, 4] (got " + std::to_string(partners) + ") and width * height * 64 below 2^31");
    if (!(p1 > 0 && p1 < p2 && p2 <= 2047)) return fail("the penalties must satisfy 0 < p1 < p2 <= 2047, got p1 " + std::to_string(p1) + ", p2 " + std::to_string(p2));
    if (uniqueness_ratio < 0 || uniqueness_ratio > 99) return fail("uniqueness_ratio must be in [0, 99], got " + std::to_string(uniqueness_ratio));
    if (min_span_px < 0) return fail("min_span_px must not be negative, got " + std::to_string(min_span_px));
    if (!(std::isfinite(w_min) && std::isfinite(w_step) && w_min >= 0.0f && w_step > 0.0f))
        return fail("w_min must be finite and >= 0 and w_step finite and > 0, got w_min " + std::to_string(w_min) + ", w_step " + std::to_string(w_step));
    if (!ref_grey || !partner_grey || !transforms || !index16 || !depth || !workspace)
        return fail("ref_grey, partner_grey, transforms, index16, depth and workspace must not be NULL");
    if (!workspace_fits("gsr_sweep_depth", "gsr_sweep_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    if (cost_sum && ((size_t)cost_sum & 1)) return fail("cost_sum must be 2-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)width * height;
    unsigned char* const C = cost ? cost : l.cost;
    unsigned short* const S = cost_sum ? cost_sum : l.cost_sum;
    const unsigned pixel_blocks = (unsigned)((n + STEREO_BLOCK - 1) / STEREO_BLOCK);
    // the census of image i (0: the reference, 1 + j: partner j) goes to codes[i]; stereo_census_kernel takes two images per launch
    auto image = [&](int i) { return i == 0 ? ref_grey : partner_grey + (size_t)(i - 1) * n; };
    for (int i = 0; i <= partners; i += 2) {
        ScopedKernelTimer tm(K_SWEEP_CENSUS, stream);
        const int pair = i + 1 <= partners ? 2 : 1;                      // an odd image out: one side, blockIdx.y stays 0
        hipLaunchKernelGGL(stereo_census_kernel, dim3(pixel_blocks, pair), dim3(STEREO_BLOCK), 0, stream, width, height, image(i),
                           pair == 2 ? image(i + 1) : nullptr, l.codes + (size_t)i * n, pair == 2 ? l.codes + (size_t)(i + 1) * n : nullptr);
        GSR_HIP_CHECK(hipGetLastError());
    }
    const unsigned wave_blocks = (unsigned)((n + STEREO_BLOCK / 64 - 1) / (STEREO_BLOCK / 64));
    {
        ScopedKernelTimer tm(K_SWEEP_COST, stream);
        hipLaunchKernelGGL(sweep_cost_kernel, dim3(wave_blocks), dim3(STEREO_BLOCK), 0, stream, width, height, partners,
                           SweepCamera{fx, fy, cx, cy, w_min, w_step}, min_span_px, l.codes, transforms, C, l.observable);
        GSR_HIP_CHECK(hipGetLastError());
    }
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    {
        ScopedKernelTimer tm(K_SWEEP_PATHS, stream);                     // the eight launches as one stage
        for (int r = 0; r < 8; ++r) {
            const int dx = dirs[r][0], dy = dirs[r][1];
            const unsigned paths = (unsigned)(dy == 0 ? height : dx == 0 ? width : width + height - 1);
            hipLaunchKernelGGL(sweep_path_kernel, dim3(paths), dim3(64), 0, stream, width, height, dx, dy, p1, p2, C, S, (int)(r == 0));
            GSR_HIP_CHECK(hipGetLastError());
        }
    }
    ScopedKernelTimer tm(K_SWEEP_SELECT, stream);
    hipLaunchKernelGGL(sweep_select_kernel, dim3(wave_blocks), dim3(STEREO_BLOCK), 0, stream, width, height, uniqueness_ratio, w_min, w_step, S,
                       l.observable, index16, depth);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// min_side: the smallest side a pyramid level may have (the pyramid: 1; the lookup divides by (side - 1): 2)
static bool raft_size_ok(const char* who, int h, int w, int min_side)
{
    if (h <= 0 || w <= 0 || (h >> 3) < min_side || (w >> 3) < min_side || (long long)h * w > 65536) {
        g_last_error = std::string(who) + ": every pyramid level must have sides of at least " + std::to_string(min_side) +
                       " and the low-res grid at most 65536 pixels";
        return false;
    }
    return true;
}

int gsr_raft_corr_pyramid(int dim, int h, int w, const float* f1, const float* f2, float* const* pyr12, float* const* pyr21, void* stream_)
{
    if (!raft_size_ok("gsr_raft_corr_pyramid", h, w, 1)) return GSR_ERR_INVALID_ARGUMENT;
    if (dim <= 0 || !f1 || !f2 || !pyr12) { g_last_error = "gsr_raft_corr_pyramid: dim must be positive and f1, f2, pyr12 given"; return GSR_ERR_INVALID_ARGUMENT; }
    for (int l = 0; l < RAFT_LEVELS; ++l)
        if (!pyr12[l] || (pyr21 && !pyr21[l])) { g_last_error = "gsr_raft_corr_pyramid: a level pointer is NULL"; return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = (hipStream_t)stream_;
    const int N = h * w;
    const unsigned tiles = (unsigned)((N + CORR_TILE - 1) / CORR_TILE);
    hipLaunchKernelGGL(raft_corr_kernel, dim3(tiles, tiles), dim3(CORR_BLOCK), 0, stream, dim, N, f1, f2, pyr12[0], pyr21 ? pyr21[0] : nullptr);
    GSR_HIP_CHECK(hipGetLastError());
    int hp = h, wp = w;
    for (int l = 1; l < RAFT_LEVELS; ++l) {
        const size_t cells = (size_t)N * (hp >> 1) * (wp >> 1);
        hipLaunchKernelGGL(raft_pool_kernel, dim3((unsigned)((cells + 255) / 256), pyr21 ? 2u : 1u), dim3(256), 0, stream, N, hp, wp,
                           pyr12[l - 1], pyr12[l], pyr21 ? pyr21[l - 1] : nullptr, pyr21 ? pyr21[l] : nullptr);
        GSR_HIP_CHECK(hipGetLastError());
        hp >>= 1;
        wp >>= 1;
    }
    return 0;
}

int gsr_raft_corr_lookup(int batch, int h, int w, const float* const* pyr, const float* coords, float* out, void* stream_)
{
    if (!raft_size_ok("gsr_raft_corr_lookup", h, w, 2)) return GSR_ERR_INVALID_ARGUMENT;
    if (batch < 1 || batch > RAFT_MAX_BATCH || !pyr || !coords || !out) {
        g_last_error = "gsr_raft_corr_lookup: batch must be 1 or 2 and pyr, coords, out given";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    RaftPyramids p{};
    for (int b = 0; b < batch; ++b)
        for (int l = 0; l < RAFT_LEVELS; ++l) {
            p.level[b][l] = pyr[b * RAFT_LEVELS + l];
            if (!p.level[b][l]) { g_last_error = "gsr_raft_corr_lookup: a level pointer is NULL"; return GSR_ERR_INVALID_ARGUMENT; }
        }
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(raft_lookup_kernel, dim3((unsigned)((h * w + 255) / 256), RAFT_LEVELS, batch), dim3(256), 0, stream, h, w, p, coords, out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_raft_upsample(int batch, int h, int w, const float* flow, const float* mask, int pad_left, int pad_top, int out_w, int out_h, int ndc,
                      float* out, void* stream_)
{
    if (batch < 1 || batch > 65535 || h <= 0 || w <= 0 || !flow || !mask || !out) {
        g_last_error = "gsr_raft_upsample: batch, h and w must be positive and flow, mask, out given";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (pad_left < 0 || pad_top < 0 || out_w <= 0 || out_h <= 0 || out_h > 65535 || pad_left + out_w > 8 * w || pad_top + out_h > 8 * h) {
        g_last_error = "gsr_raft_upsample: the crop window must lie inside the 8h x 8w upsampled flow";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(raft_upsample_kernel, dim3((unsigned)((out_w + 255) / 256), out_h, batch), dim3(256), 0, stream, h, w, flow, mask, pad_left,
                       pad_top, out_w, out_h, ndc, out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

static bool gma_args_ok(const char* who, int batch, int dim, int h, int w, bool pointers)
{
    if (batch < 1 || batch > GMA_MAX_BATCH || dim <= 0 || dim % 4 != 0 || h < 1 || w < 1 || (long long)h * w > 65535) {
        g_last_error = std::string(who) + ": batch must be 1 or 2, dim a positive multiple of 4, h and w at least 1 and h * w at most 65535 (got batch " +
                       std::to_string(batch) + ", dim " + std::to_string(dim) + ", " + std::to_string(h) + " x " + std::to_string(w) + ")";
        return false;
    }
    if (!pointers) { g_last_error = std::string(who) + ": a pointer is NULL"; return false; }
    return true;
}

int gsr_gma_attention(int batch, int dim, int h, int w, const float* q, const float* k, float scale, float* attn, void* stream_)
{
    if (!gma_args_ok("gsr_gma_attention", batch, dim, h, w, q && k && attn)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = h * w;
    const unsigned tiles = (unsigned)((N + GMA_TILE - 1) / GMA_TILE);
    hipLaunchKernelGGL(gma_sim_kernel, dim3(tiles, tiles, batch), dim3(GMA_BLOCK), 0, stream, dim, N, q, k, scale, attn);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(gma_softmax_kernel, dim3(N, batch), dim3(GMA_BLOCK), 0, stream, N, attn);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_gma_aggregate(int batch, int dim, int h, int w, const float* attn, const float* v, const float* x, float gamma, float* out, void* stream_)
{
    if (!gma_args_ok("gsr_gma_aggregate", batch, dim, h, w, attn && v && x && out)) return GSR_ERR_INVALID_ARGUMENT;
    if (out == x || out == v) { g_last_error = "gsr_gma_aggregate: out must not alias x or v"; return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = (hipStream_t)stream_;
    const int N = h * w;
    hipLaunchKernelGGL(gma_aggregate_kernel, dim3((unsigned)((N + GMA_TILE - 1) / GMA_TILE), (unsigned)((dim + GMA_TILE - 1) / GMA_TILE), batch),
                       dim3(GMA_AGG_THREADS), 0, stream, dim, N, attn, v, x, gamma, out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_yolo_detect: score [A] | cls [A] | box float4 [A] | order [A] | obox float4 [A] | n | mask u64 [A, words]
struct YoloWs { float* score; int* cls; float4* box; int* order; float4* obox; int* n; unsigned long long* mask; size_t bytes; };
static YoloWs yolo_layout(size_t A, const void* workspace)
{
    Carver c(workspace, 256);
    return {c.take<float>(A), c.take<int>(A), c.take<float4>(A), c.take<int>(A), c.take<float4>(A), c.take<int>(1),
            c.take<unsigned long long>(A * ((A + 63) / 64)), c.bytes()};
}
size_t gsr_yolo_workspace_size(int anchors) { return anchors > 0 && anchors <= YOLO_MAX_ANCHORS ? yolo_layout((size_t)anchors, nullptr).bytes : 0; }

int gsr_yolo_detect(int levels, const int* level_hw, const float* level_stride, const float* const* head, const float* const* coef, int nc,
                    int nm, const int* classes, int n_classes, float conf, float iou, int max_det, void* workspace, float* dets, int max_dets,
                    int* counts, void* stream_)
{
    if (levels < 1 || levels > YOLO_MAX_LEVELS || !level_hw || !level_stride || !head || !coef || !classes || !workspace || !dets || !counts) {
        g_last_error = "gsr_yolo_detect: 1 to 4 levels, and level_hw, level_stride, head, coef, classes, workspace, dets, counts given";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (nc < 1 || nc > YOLO_MAX_CLASSES || nm < 1 || nm > YOLO_MAX_NM || n_classes < 1 || max_det < 1 || max_dets < 1 || !(conf >= 0.f) ||
        !(iou >= 0.f)) {
        g_last_error = "gsr_yolo_detect: needs 1 <= nc <= 256, 1 <= nm <= 64, at least one class, max_det, max_dets >= 1, conf, iou >= 0";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    YoloLevels L{};
    L.levels = levels;
    long long A = 0;
    for (int l = 0; l < levels; ++l) {
        L.h[l] = level_hw[2 * l];
        L.w[l] = level_hw[2 * l + 1];
        L.head[l] = head[l];
        L.coef[l] = coef[l];
        L.stride[l] = level_stride[l];
        L.first[l] = (int)A;
        if (L.h[l] < 1 || L.w[l] < 1 || !head[l] || !coef[l] || !(level_stride[l] > 0.f)) {
            g_last_error = "gsr_yolo_detect: a level has an empty grid, a NULL tensor or a stride that is not positive";
            return GSR_ERR_INVALID_ARGUMENT;
        }
        A += (long long)L.h[l] * L.w[l];
        if (A > YOLO_MAX_ANCHORS) {
            g_last_error = "gsr_yolo_detect: more than " + std::to_string(YOLO_MAX_ANCHORS) + " anchors (the sort's LDS capacity)";
            return GSR_ERR_INVALID_ARGUMENT;
        }
    }
    L.first[levels] = (int)A;
    YoloClassSet cs{};
    for (int k = 0; k < n_classes; ++k) {
        if (classes[k] < 0 || classes[k] >= nc) { g_last_error = "gsr_yolo_detect: a class id is outside [0, nc)"; return GSR_ERR_INVALID_ARGUMENT; }
        cs.bits[classes[k] >> 5] |= 1u << (classes[k] & 31);
    }
    const int words = (int)((A + 63) / 64);
    const auto [score, cls, box, order, obox, n, mask, ws_bytes] = yolo_layout((size_t)A, workspace);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(yolo_decode_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, stream, L, (int)A, nc, cs, conf, score, cls, box);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(yolo_sort_kernel, dim3(1), dim3(YOLO_SORT_BLOCK), 0, stream, (int)A, score, cls, box, order, obox, n);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(yolo_iou_kernel, dim3((unsigned)words, (unsigned)words), dim3(64), 0, stream, n, obox, iou, words, mask);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(yolo_select_kernel, dim3(1), dim3(64), 0, stream, L, n, order, score, cls, box, mask, words, nc, nm, max_det, max_dets,
                       dets, counts);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_yolo_masks(int max_dets, const float* dets, const int* counts, int nm, const float* proto, int proto_h, int proto_w, int height, int width,
                   unsigned char* yolo_mask, unsigned char* motion, void* stream_)
{
    if (max_dets < 0 || !dets || !counts || !proto || nm < 1 || nm > YOLO_MAX_NM || (!yolo_mask && !motion)) {
        g_last_error = "gsr_yolo_masks: dets, counts, proto and an output given, 1 <= nm <= 64";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (height <= 0 || width <= 0 || height % YOLO_TILE || width % YOLO_TILE || proto_h * 4 != height || proto_w * 4 != width ||
        (long long)height * width > 0x7fffffffLL) {
        g_last_error = "gsr_yolo_masks: height and width must be positive multiples of 32 and the proto exactly a quarter of them";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(yolo_mask_kernel, dim3((unsigned)(width / YOLO_TILE), (unsigned)(height / YOLO_TILE)), dim3(256), 0, stream, counts,
                       max_dets, dets, nm, proto, proto_h, proto_w, height, width, yolo_mask, motion);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// levels, shapes and the block layout of a distance call; false (with the error text set) when an argument is out of range
static bool lpips_levels(const char* who, int batch, int levels, const int* level_chw, LpipsLevels& L)
{
    if (batch < 1 || batch > 65535 || levels < 1 || levels > LPIPS_MAX_LEVELS || !level_chw) {
        g_last_error = std::string(who) + ": 1 <= batch <= 65535, 1 to " + std::to_string(LPIPS_MAX_LEVELS) + " levels and level_chw given";
        return false;
    }
    L.levels = levels;
    long long blocks = 0;
    for (int l = 0; l < levels; ++l) {
        const long long c = level_chw[3 * l], h = level_chw[3 * l + 1], w = level_chw[3 * l + 2];
        if (c < 1 || h < 1 || w < 1 || h * w > 0x7fffffffLL - LPIPS_BLOCK || c > 65536) {
            g_last_error = std::string(who) + ": a level has no channels or pixels, more than 65536 channels or 2^31 pixels";
            return false;
        }
        L.c[l] = (int)c;
        L.hw[l] = (int)(h * w);
        L.blocks[l] = (int)((h * w + LPIPS_BLOCK - 1) / LPIPS_BLOCK);
        L.first[l] = (int)blocks;
        blocks += (long long)batch * L.blocks[l];
        if (blocks > 0x7fffffffLL) { g_last_error = std::string(who) + ": more than 2^31 blocks"; return false; }
    }
    L.first[levels] = (int)blocks;
    return true;
}

int gsr_lpips_prepare(int batch, int height, int width, const float* x, const float* y, float* out, void* stream_)
{
    if (!x || !y || !out) { g_last_error = "gsr_lpips_prepare: x, y and out must not be NULL"; return GSR_ERR_INVALID_ARGUMENT; }
    if (batch < 1 || height < 1 || width < 1 || (long long)batch * 6 * height * width > 0x7fffffffLL) {
        g_last_error = "gsr_lpips_prepare: batch, height and width must be positive and 2 * batch * 3 * height * width below 2^31";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int hw = height * width, n = batch * 3 * hw;
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3((unsigned)((n + LPIPS_PREPARE_BLOCK - 1) / LPIPS_PREPARE_BLOCK)), dim3(LPIPS_PREPARE_BLOCK), 0,
                       (hipStream_t)stream_, n, hw, x, y, out);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace: one float per block of the distance launch
size_t gsr_lpips_workspace_size(int batch, int levels, const int* level_chw)
{
    LpipsLevels L{};
    if (!lpips_levels("gsr_lpips_workspace_size", batch, levels, level_chw, L)) return 0;
    return (size_t)L.first[levels] * sizeof(float);
}

int gsr_lpips_distance(int batch, int levels, const int* level_chw, const float* const* feat, const float* const* lin, int norm,
                       void* workspace, float* taps, float* scores, void* stream_)
{
    LpipsLevels L{};
    if (!lpips_levels("gsr_lpips_distance", batch, levels, level_chw, L)) return GSR_ERR_INVALID_ARGUMENT;
    if (!feat || !lin || !workspace || !scores || (norm != LPIPS_NORM_TORCHMETRICS && norm != LPIPS_NORM_LPIPS)) {
        g_last_error = "gsr_lpips_distance: feat, lin, workspace and scores given, norm one of GSR_LPIPS_NORM_*";
        return GSR_ERR_INVALID_ARGUMENT;
    }
    for (int l = 0; l < levels; ++l) {
        if (!feat[l] || !lin[l]) { g_last_error = "gsr_lpips_distance: a level's feat or lin pointer is NULL"; return GSR_ERR_INVALID_ARGUMENT; }
        L.feat[l] = feat[l];
        L.lin[l] = lin[l];
    }
    hipStream_t stream = (hipStream_t)stream_;
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(lpips_distance_kernel, dim3((unsigned)L.first[levels]), dim3(LPIPS_BLOCK), 0, stream, L, batch, norm, partial);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)batch), dim3(64), 0, stream, L, partial, taps, scores);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_flow_rigid_fit: MotionHead | flags [H, W] bytes | the slab [blocks, 32] doubles; every part starts on a multiple of 16 bytes
struct MotionFitLayout { MotionHead* head; unsigned char* flags; double* slab; size_t bytes; unsigned blocks; };
static bool motion_size_ok(int width, int height)
{
    return width >= 1 && height >= 1 && (long long)width * height < 0x80000000LL;
}
static bool motion_fit_layout(int width, int height, const void* workspace, MotionFitLayout& l)
{
    if (!motion_size_ok(width, height)) return false;
    const size_t n = (size_t)width * height;
    l.blocks = (unsigned)std::min<size_t>((n + MOTION_BLOCK - 1) / MOTION_BLOCK, MOTION_MAX_BLOCKS);
    Carver c(workspace, 16);
    l.head = c.take<MotionHead>(1);
    l.flags = c.take<unsigned char>(n);
    l.slab = c.take<double>((size_t)l.blocks * MOTION_ROW);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_flow_rigid_fit_workspace_size(int width, int height) { MotionFitLayout l; return motion_fit_layout(width, height, nullptr, l) ? l.bytes : 0; }

int gsr_flow_rigid_fit(int width, int height, float fx, float fy, float cx, float cy, const float* flow_ij, const float* depth_i,
                       const float* flow_ji, const unsigned char* fit_mask, const float* T_init, int iters, float scale_multiplier,
                       float c_min, float c_max, float occlusion_px, float residual_px, float* T, float* residual, double* stats,
                       unsigned char* candidate, double* trace, void* workspace, size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_flow_rigid_fit: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    MotionFitLayout l;
    if (!motion_fit_layout(width, height, workspace, l)) return fail("width and height must be positive and width * height below 2^31");
    if (!(fx > 0.f && fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("fx and fy must be positive and the intrinsics finite");
    if (iters < 1 || iters > 64) return fail("iters must be in [1, 64], got " + std::to_string(iters));
    if (!(scale_multiplier > 0.f) || !(c_min > 0.f) || !(c_max >= c_min) || !std::isfinite(c_max) || !std::isfinite(scale_multiplier))
        return fail("scale_multiplier must be positive and 0 < c_min <= c_max");
    if (!(occlusion_px >= 0.f) || !(residual_px >= 0.f)) return fail("occlusion_px and residual_px must not be negative");
    if (!flow_ij || !depth_i || !T || !residual || !stats || !workspace)
        return fail("flow_ij, depth_i, T, residual, stats and workspace must not be NULL");
    if (!workspace_fits("gsr_flow_rigid_fit", "gsr_flow_rigid_fit_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    MotionHead* const head = l.head;
    unsigned char* const flags = l.flags;
    double* const slab = l.slab;
    const MotionCam cam{width, height, fx, fy, cx, cy};
    const size_t n = (size_t)width * height;
    const unsigned pixel_blocks = (unsigned)((n + MOTION_BLOCK - 1) / MOTION_BLOCK);
    const float2* f_ij = reinterpret_cast<const float2*>(flow_ij);
    GSR_HIP_CHECK(hipMemsetAsync(head, 0, flags - reinterpret_cast<unsigned char*>(head), stream));
    hipLaunchKernelGGL(motion_prep_kernel, dim3(pixel_blocks), dim3(MOTION_BLOCK), 0, stream, cam, f_ij, depth_i,
                       reinterpret_cast<const float2*>(flow_ji), fit_mask, T_init, occlusion_px, flags, head);
    GSR_HIP_CHECK(hipGetLastError());
    for (int k = 0; k < iters; ++k) {
        hipLaunchKernelGGL(motion_residual_kernel, dim3(l.blocks), dim3(MOTION_BLOCK), 0, stream, cam, f_ij, depth_i, flags, head, (float*)nullptr);
        GSR_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(motion_normal_kernel, dim3(l.blocks), dim3(MOTION_BLOCK), 0, stream, cam, f_ij, depth_i, flags, head, scale_multiplier,
                           c_min, c_max, slab);
        GSR_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(motion_solve_kernel, dim3(1), dim3(MOTION_BLOCK), 0, stream, (int)l.blocks, slab, head,
                           trace ? trace + (size_t)k * MOTION_ROW : (double*)nullptr);
        GSR_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(motion_residual_kernel, dim3(l.blocks), dim3(MOTION_BLOCK), 0, stream, cam, f_ij, depth_i, flags, head, residual);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_finish_kernel, dim3(candidate ? pixel_blocks : 1u), dim3(MOTION_BLOCK), 0, stream, (long long)n, head, scale_multiplier,
                       c_min, c_max, residual_px, flags, residual, T, stats, candidate);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_motion_mask_clean: two byte images [H, W] | parent [H, W] int32 | area [H, W] int32
struct MotionCleanLayout { unsigned char *a, *b; int *parent, *area; size_t bytes; };
static bool motion_clean_layout(int width, int height, const void* workspace, MotionCleanLayout& l)
{
    if (!motion_size_ok(width, height)) return false;
    const size_t n = (size_t)width * height;
    Carver c(workspace, 16);
    l.a = c.take<unsigned char>(n);
    l.b = c.take<unsigned char>(n);
    l.parent = c.take<int>(n);
    l.area = c.take<int>(n);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_motion_mask_clean_workspace_size(int width, int height) { MotionCleanLayout l; return motion_clean_layout(width, height, nullptr, l) ? l.bytes : 0; }

int gsr_motion_mask_clean(int width, int height, const unsigned char* candidate, int open_radius, int grow_radius, int min_area,
                          unsigned char* moving, int* labels, int* counts, unsigned char* motion, void* workspace, size_t workspace_bytes,
                          void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_motion_mask_clean: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    MotionCleanLayout l;
    if (!motion_clean_layout(width, height, workspace, l)) return fail("width and height must be positive and width * height below 2^31");
    if (open_radius < 0 || open_radius > 8 || grow_radius < 0 || grow_radius > 8)
        return fail("open_radius and grow_radius must be in [0, 8], got " + std::to_string(open_radius) + " and " + std::to_string(grow_radius));
    if (min_area < 1) return fail("min_area must be at least 1, got " + std::to_string(min_area));
    if (!candidate || !moving || !labels || !counts || !workspace) return fail("candidate, moving, labels, counts and workspace must not be NULL");
    if (!workspace_fits("gsr_motion_mask_clean", "gsr_motion_mask_clean_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* const a = l.a, * const b = l.b;
    int* const parent = l.parent, * const area = l.area;
    const long long n = (long long)width * height;
    const dim3 grid((unsigned)((n + MOTION_BLOCK - 1) / MOTION_BLOCK)), block(MOTION_BLOCK);
    hipLaunchKernelGGL(motion_morph_kernel, grid, block, 0, stream, width, height, open_radius, 1, candidate, a, (unsigned char*)nullptr, (int*)nullptr);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_morph_kernel, grid, block, 0, stream, width, height, open_radius, 0, (const unsigned char*)a, b, (unsigned char*)nullptr,
                       (int*)nullptr);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_label_init_kernel, grid, block, 0, stream, width, n, (const unsigned char*)b, parent, area, counts);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_label_merge_kernel, grid, block, 0, stream, width, height, (const unsigned char*)b, parent);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_label_flatten_kernel, grid, block, 0, stream, n, parent, labels);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_label_count_kernel, grid, block, 0, stream, n, (const int*)labels, area, counts);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_label_filter_kernel, grid, block, 0, stream, n, min_area, (const int*)area, labels, a, counts);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(motion_morph_kernel, grid, block, 0, stream, width, height, grow_radius, 0, (const unsigned char*)a, moving, motion, counts + 3);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// a pyramid buffer of gsr_odometry_pyramid: OdoPyramidHead | per level I [h, w] floats | D [h, w] floats; every part starts on a multiple of 16 bytes
struct OdoPyramidLayout { OdoPyramidHead* head; int w[ODO_MAX_LEVELS], h[ODO_MAX_LEVELS]; float* I[ODO_MAX_LEVELS]; float* D[ODO_MAX_LEVELS]; size_t bytes; };
static bool odo_pyramid_layout(int width, int height, int levels, const void* buffer, OdoPyramidLayout& l)
{
    if (width < 1 || height < 1 || levels < 1 || levels > ODO_MAX_LEVELS || (long long)width * height >= 0x80000000LL) return false;
    if ((width >> (levels - 1)) < ODO_MIN_COARSEST || (height >> (levels - 1)) < ODO_MIN_COARSEST) return false;
    Carver c(buffer, 16);
    l.head = c.take<OdoPyramidHead>(1);
    for (int k = 0; k < levels; ++k) {
        l.w[k] = width >> k;
        l.h[k] = height >> k;
        l.I[k] = c.take<float>((size_t)l.w[k] * l.h[k]);
        l.D[k] = c.take<float>((size_t)l.w[k] * l.h[k]);
    }
    l.bytes = c.bytes_padded();
    return true;
}
static const char* const kOdoSizeText = "levels must be in [1, 6], the coarsest level at least 8 x 8 and width * height below 2^31";

size_t gsr_odometry_pyramid_size(int width, int height, int levels)
{
    OdoPyramidLayout l;
    return odo_pyramid_layout(width, height, levels, nullptr, l) ? l.bytes : 0;
}

int gsr_odometry_pyramid(int width, int height, int levels, const float* image, const float* depth, const unsigned char* mask,
                         float depth_min, float depth_max, void* pyramid, size_t pyramid_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_odometry_pyramid: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    OdoPyramidLayout l;
    if (!odo_pyramid_layout(width, height, levels, pyramid, l)) return fail(kOdoSizeText);
    if (!(depth_min >= 0.f) || !(depth_max >= depth_min)) return fail("0 <= depth_min <= depth_max must hold");
    if (!image || !pyramid) return fail("image and pyramid must not be NULL");
    if (!workspace_fits("gsr_odometry_pyramid", "gsr_odometry_pyramid_size", pyramid, pyramid_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    ScopedKernelTimer tm(K_ODO_PYRAMID, stream);
    GSR_HIP_CHECK(hipMemsetAsync(l.head, 0, sizeof(OdoPyramidHead), stream));
    auto blocks = [](int w, int h) { return dim3((unsigned)(((size_t)w * h + ODO_BLOCK - 1) / ODO_BLOCK)); };
    hipLaunchKernelGGL(odo_level0_kernel, blocks(width, height), dim3(ODO_BLOCK), 0, stream, width, height, image, depth, mask, depth_min,
                       depth_max, l.I[0], l.D[0], l.head);
    GSR_HIP_CHECK(hipGetLastError());
    for (int k = 1; k < levels; ++k) {
        hipLaunchKernelGGL(odo_down_kernel, blocks(l.w[k], l.h[k]), dim3(ODO_BLOCK), 0, stream, l.w[k], l.h[k], l.w[k - 1], (const float*)l.I[k - 1],
                           (const float*)l.D[k - 1], l.I[k], l.D[k]);
        GSR_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// workspace of gsr_odometry_align: OdoHead | the slab [blocks of level 0, 32] doubles
struct OdoAlignLayout { OdoHead* head; double* slab; size_t bytes; };
static unsigned odo_blocks(int w, int h) { return (unsigned)std::min<size_t>(((size_t)w * h + ODO_BLOCK - 1) / ODO_BLOCK, ODO_MAX_BLOCKS); }
static bool odo_align_layout(int width, int height, int levels, const void* workspace, OdoAlignLayout& l)
{
    OdoPyramidLayout p;
    if (!odo_pyramid_layout(width, height, levels, nullptr, p)) return false;
    Carver c(workspace, 16);
    l.head = c.take<OdoHead>(1);
    l.slab = c.take<double>((size_t)odo_blocks(width, height) * MOTION_ROW);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_odometry_align_workspace_size(int width, int height, int levels)
{
    OdoAlignLayout l;
    return odo_align_layout(width, height, levels, nullptr, l) ? l.bytes : 0;
}

int gsr_odometry_align(int width, int height, int levels, float fx, float fy, float cx, float cy, const void* previous, const void* current,
                       const float* T_init, const int* iters, float nu, float sigma_init, float sigma_min, float min_share, float max_last_step,
                       float max_translation, float max_rotation, float* T, double* stats, double* trace, void* workspace,
                       size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_odometry_align: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    OdoAlignLayout l;
    OdoPyramidLayout P, C;
    if (!odo_align_layout(width, height, levels, workspace, l) || !odo_pyramid_layout(width, height, levels, previous, P) ||
        !odo_pyramid_layout(width, height, levels, current, C))
        return fail(kOdoSizeText);
    if (!(fx > 0.f && fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("fx and fy must be positive and the intrinsics finite");
    if (!iters) return fail("iters must not be NULL");
    for (int k = 0; k < levels; ++k)
        if (iters[k] < 0 || iters[k] > 64) return fail("iters[" + std::to_string(k) + "] must be in [0, 64], got " + std::to_string(iters[k]));
    if (!(nu > 0.f) || !std::isfinite(nu) || !(sigma_init > 0.f) || !std::isfinite(sigma_init) || !(sigma_min > 0.f) || !std::isfinite(sigma_min))
        return fail("nu, sigma_init and sigma_min must be positive and finite");
    if (!(min_share >= 0.f && min_share <= 1.f) || !(max_last_step >= 0.f) || !(max_translation >= 0.f) || !(max_rotation >= 0.f))
        return fail("min_share must be in [0, 1] and max_last_step, max_translation, max_rotation must not be negative");
    if (!previous || !current || !T || !stats || !workspace) return fail("previous, current, T, stats and workspace must not be NULL");
    if (!workspace_fits("gsr_odometry_align", "gsr_odometry_align_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    {
        ScopedKernelTimer tm(K_ODO_SOLVE, stream);
        hipLaunchKernelGGL(odo_init_kernel, dim3(1), dim3(64), 0, stream, T_init, sigma_init, l.head);
        GSR_HIP_CHECK(hipGetLastError());
    }
    int pass = 0;
    for (int k = levels - 1; k >= 0; --k) {
        const float scale = 1.f / (float)(1 << k);                                  // a power of two: the products below are exact
        const OdoLevel L{P.w[k], P.h[k], fx * scale, fy * scale, (float)(((double)cx + 0.5) * scale - 0.5), (float)(((double)cy + 0.5) * scale - 0.5),
                         P.I[k], P.D[k], C.I[k]};
        const unsigned blocks = odo_blocks(L.w, L.h);
        for (int it = 0; it < iters[k]; ++it, ++pass) {
            {
                ScopedKernelTimer tm(K_ODO_SUMS, stream);
                hipLaunchKernelGGL(odo_sums_kernel, dim3(blocks), dim3(ODO_BLOCK), 0, stream, L, nu, (const OdoHead*)l.head, l.slab);
                GSR_HIP_CHECK(hipGetLastError());
            }
            ScopedKernelTimer tm(K_ODO_SOLVE, stream);
            hipLaunchKernelGGL(odo_solve_kernel, dim3(1), dim3(ODO_BLOCK), 0, stream, (int)blocks, (const double*)l.slab, l.head, sigma_min, k,
                               trace ? trace + (size_t)pass * MOTION_ROW : (double*)nullptr);
            GSR_HIP_CHECK(hipGetLastError());
        }
    }
    ScopedKernelTimer tm(K_ODO_SOLVE, stream);
    hipLaunchKernelGGL(odo_finish_kernel, dim3(1), dim3(64), 0, stream, (const OdoHead*)l.head, (const OdoPyramidHead*)P.head, min_share, max_last_step,
                       max_translation, max_rotation, T, stats);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_odometry_align_rgbd: OdoRgbdHead | the slab [blocks of level 0, 64] doubles
struct OdoRgbdLayout { OdoRgbdHead* head; double* slab; size_t bytes; };
static bool odo_rgbd_layout(int width, int height, int levels, const void* workspace, OdoRgbdLayout& l)
{
    OdoPyramidLayout p;
    if (!odo_pyramid_layout(width, height, levels, nullptr, p)) return false;
    Carver c(workspace, 16);
    l.head = c.take<OdoRgbdHead>(1);
    l.slab = c.take<double>((size_t)odo_blocks(width, height) * ODO_RGBD_ROW);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_odometry_align_rgbd_workspace_size(int width, int height, int levels)
{
    OdoRgbdLayout l;
    return odo_rgbd_layout(width, height, levels, nullptr, l) ? l.bytes : 0;
}

int gsr_odometry_align_rgbd(int width, int height, int levels, float fx, float fy, float cx, float cy, const void* previous, const void* current,
                            const float* T_init, const int* iters, int affine, float geometric_weight, float edge_ratio, float nu, float sigma_init,
                            float sigma_min, float sigma_depth_init, float sigma_depth_min, float min_share, float max_last_step,
                            float max_translation, float max_rotation, float max_gain, float max_offset, float* T, double* stats, double* trace,
                            void* workspace, size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_odometry_align_rgbd: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    OdoRgbdLayout l;
    OdoPyramidLayout P, C;
    if (!odo_rgbd_layout(width, height, levels, workspace, l) || !odo_pyramid_layout(width, height, levels, previous, P) ||
        !odo_pyramid_layout(width, height, levels, current, C))
        return fail(kOdoSizeText);
    if (!(fx > 0.f && fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("fx and fy must be positive and the intrinsics finite");
    if (!iters) return fail("iters must not be NULL");
    for (int k = 0; k < levels; ++k)
        if (iters[k] < 0 || iters[k] > 64) return fail("iters[" + std::to_string(k) + "] must be in [0, 64], got " + std::to_string(iters[k]));
    if (affine != 0 && affine != 1) return fail("affine must be 0 or 1, got " + std::to_string(affine));
    if (!(geometric_weight >= 0.f) || !std::isfinite(geometric_weight) || !(edge_ratio >= 0.f) || !std::isfinite(edge_ratio))
        return fail("geometric_weight and edge_ratio must be finite and not negative");
    if (!(nu > 0.f) || !std::isfinite(nu) || !(sigma_init > 0.f) || !std::isfinite(sigma_init) || !(sigma_min > 0.f) || !std::isfinite(sigma_min))
        return fail("nu, sigma_init and sigma_min must be positive and finite");
    if (!(sigma_depth_init > 0.f) || !std::isfinite(sigma_depth_init) || !(sigma_depth_min > 0.f) || !std::isfinite(sigma_depth_min))
        return fail("sigma_depth_init and sigma_depth_min must be positive and finite");
    if (!(min_share >= 0.f && min_share <= 1.f) || !(max_last_step >= 0.f) || !(max_translation >= 0.f) || !(max_rotation >= 0.f))
        return fail("min_share must be in [0, 1] and max_last_step, max_translation, max_rotation must not be negative");
    if (!(max_gain >= 0.f) || !(max_offset >= 0.f)) return fail("max_gain and max_offset must not be negative");
    if (!previous || !current || !T || !stats || !workspace) return fail("previous, current, T, stats and workspace must not be NULL");
    if (!workspace_fits("gsr_odometry_align_rgbd", "gsr_odometry_align_rgbd_workspace_size", workspace, workspace_bytes, l.bytes))
        return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    {
        ScopedKernelTimer tm(K_ODO_SOLVE, stream);
        hipLaunchKernelGGL(odo_rgbd_init_kernel, dim3(1), dim3(64), 0, stream, T_init, sigma_init, sigma_depth_init, l.head);
        GSR_HIP_CHECK(hipGetLastError());
    }
    const bool depth_term = geometric_weight > 0.f;
    int pass = 0;
    for (int k = levels - 1; k >= 0; --k) {
        const float scale = 1.f / (float)(1 << k);                                  // a power of two: the products below are exact
        const OdoRgbdLevel L{P.w[k], P.h[k], fx * scale, fy * scale, (float)(((double)cx + 0.5) * scale - 0.5),
                             (float)(((double)cy + 0.5) * scale - 0.5), P.I[k], P.D[k], C.I[k], C.D[k]};
        const unsigned blocks = odo_blocks(L.w, L.h);
        for (int it = 0; it < iters[k]; ++it, ++pass) {
            double* const row = trace ? trace + (size_t)pass * ODO_RGBD_ROW : (double*)nullptr;
            auto launch = [&](auto A, auto D) {                                     // the instantiation without the terms that are off
                constexpr bool AFFINE = decltype(A)::value, DEPTH = decltype(D)::value;
                {
                    ScopedKernelTimer tm(K_ODO_SUMS, stream);
                    hipLaunchKernelGGL((odo_rgbd_sums_kernel<AFFINE, DEPTH>), dim3(blocks), dim3(ODO_BLOCK), 0, stream, L, nu, geometric_weight,
                                       edge_ratio, (const OdoRgbdHead*)l.head, l.slab);
                }
                ScopedKernelTimer tm(K_ODO_SOLVE, stream);
                hipLaunchKernelGGL((odo_rgbd_solve_kernel<AFFINE ? 8 : 6>), dim3(1), dim3(ODO_BLOCK), 0, stream, (int)blocks, (const double*)l.slab,
                                   l.head, sigma_min, sigma_depth_min, k, row);
            };
            if (affine && depth_term) launch(std::true_type{}, std::true_type{});
            else if (affine) launch(std::true_type{}, std::false_type{});
            else if (depth_term) launch(std::false_type{}, std::true_type{});
            else launch(std::false_type{}, std::false_type{});
            GSR_HIP_CHECK(hipGetLastError());
        }
    }
    ScopedKernelTimer tm(K_ODO_SOLVE, stream);
    hipLaunchKernelGGL(odo_rgbd_finish_kernel, dim3(1), dim3(64), 0, stream, (const OdoRgbdHead*)l.head, (const OdoPyramidHead*)P.head, affine,
                       min_share, max_last_step, max_translation, max_rotation, max_gain, max_offset, T, stats);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_reloc_encode: the sums of every cell, [grid_w * grid_h, 6] words
struct RelocEncodeLayout { unsigned* cells; size_t bytes; };
static bool reloc_encode_layout(int grid_w, int grid_h, const void* workspace, RelocEncodeLayout& l)
{
    if (grid_w < 1 || grid_h < 1 || (long long)grid_w * grid_h > RELOC_MAX_CELLS) return false;
    Carver c(workspace, 16);
    l.cells = c.take<unsigned>((size_t)grid_w * grid_h * RELOC_CELL_WORDS);
    l.bytes = c.bytes_padded();
    return true;
}
static bool reloc_ferns_ok(int ferns) { return ferns >= 8 && ferns <= RELOC_MAX_FERNS && ferns % 8 == 0; }

size_t gsr_reloc_encode_workspace_size(int grid_w, int grid_h)
{
    RelocEncodeLayout l;
    return reloc_encode_layout(grid_w, grid_h, nullptr, l) ? l.bytes : 0;
}

int gsr_reloc_encode(int width, int height, const float* image, const float* depth, const unsigned char* mask, int grid_w, int grid_h,
                     int ferns, const int* fern_table, float depth_scale, unsigned int* code, void* workspace, size_t workspace_bytes,
                     void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_reloc_encode: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    RelocEncodeLayout l;
    if (width < 1 || height < 1 || (long long)width * height >= (1LL << 23))
        return fail("width and height must be at least 1 and width * height below 2^23, got " + std::to_string(width) + " x " + std::to_string(height));
    if (!reloc_encode_layout(grid_w, grid_h, workspace, l) || grid_w > width || grid_h > height)
        return fail("1 <= grid_w <= width, 1 <= grid_h <= height and grid_w * grid_h <= 4096 must hold, got " + std::to_string(grid_w) + " x " +
                    std::to_string(grid_h));
    if (!reloc_ferns_ok(ferns)) return fail("ferns must be a multiple of 8 in [8, 2048], got " + std::to_string(ferns));
    if (!(depth_scale > 0.f) || !std::isfinite(depth_scale)) return fail("depth_scale must be positive and finite");
    if (!image || !fern_table || !code || !workspace) return fail("image, fern_table, code and workspace must not be NULL");
    if (!workspace_fits("gsr_reloc_encode", "gsr_reloc_encode_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const int cells = grid_w * grid_h;
    hipLaunchKernelGGL(reloc_cells_kernel, dim3((unsigned)cells), dim3(RELOC_BLOCK), 0, stream, width, height, image, depth, mask, grid_w, grid_h,
                       depth_scale, l.cells);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(reloc_ferns_kernel, dim3(1), dim3(RELOC_BLOCK), 0, stream, ferns, cells, fern_table, (const unsigned*)l.cells, code);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_reloc_search(int rows, int ferns, const unsigned int* database, const unsigned int* query, int nibble_mask, int topk, int* distance,
                     int* best, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_reloc_search: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    if (rows < 0 || rows > RELOC_MAX_ROWS) return fail("rows must be in [0, 2^20], got " + std::to_string(rows));
    if (!reloc_ferns_ok(ferns)) return fail("ferns must be a multiple of 8 in [8, 2048], got " + std::to_string(ferns));
    if (nibble_mask < 1 || nibble_mask > 15) return fail("nibble_mask must be in [1, 15], got " + std::to_string(nibble_mask));
    if (topk < 1 || topk > RELOC_MAX_TOPK) return fail("topk must be in [1, 16], got " + std::to_string(topk));
    if (!best) return fail("best must not be NULL");
    if (rows > 0 && (!database || !query || !distance)) return fail("database, query and distance must not be NULL when rows > 0");
    hipStream_t stream = (hipStream_t)stream_;
    if (rows > 0) {
        const int words = ferns / 8;
        int lanes = 1;
        while (lanes < words && lanes < 64) lanes <<= 1;
        const size_t threads = (size_t)rows * lanes;
        hipLaunchKernelGGL(reloc_distance_kernel, dim3((unsigned)((threads + RELOC_BLOCK - 1) / RELOC_BLOCK)), dim3(RELOC_BLOCK), 0, stream, rows,
                           words, lanes, database, query, (unsigned)nibble_mask * 0x11111111u, distance);
        GSR_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(reloc_select_kernel, dim3(1), dim3(RELOC_SELECT_BLOCK), 0, stream, rows, ferns, topk, (const int*)distance, best);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_reloc_score(int width, int height, const float* render, const float* render_depth, const float* opacity, const float* image,
                    const float* depth, const unsigned char* mask, int tau_colour, float tau_depth, int* counts, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_reloc_score: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    if (width < 1 || height < 1 || (long long)width * height >= 0x80000000LL)
        return fail("width and height must be at least 1 and width * height below 2^31, got " + std::to_string(width) + " x " + std::to_string(height));
    if (tau_colour < 0 || tau_colour > 765) return fail("tau_colour must be in [0, 765], got " + std::to_string(tau_colour));
    if (!(tau_depth >= 0.f) || !std::isfinite(tau_depth)) return fail("tau_depth must be finite and not negative");
    if (!render || !render_depth || !opacity || !image || !counts) return fail("render, render_depth, opacity, image and counts must not be NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)width * height;
    GSR_HIP_CHECK(hipMemsetAsync(counts, 0, RELOC_COUNTS * sizeof(int), stream));
    const unsigned blocks = (unsigned)std::min<size_t>((n + RELOC_BLOCK - 1) / RELOC_BLOCK, RELOC_SCORE_MAX_BLOCKS);
    hipLaunchKernelGGL(reloc_score_kernel, dim3(blocks), dim3(RELOC_BLOCK), 0, stream, n, render, render_depth, opacity, image, depth, mask, tau_colour,
                       tau_depth, counts);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_pose_graph_solve: the old poses, per edge its residual and Jacobian blocks and the two contributions of a product, the
// vectors of the conjugate gradients, per node the damping and the Cholesky factor of its block, the sorted keys and the node lists
static bool pose_graph_layout(int nodes, int edges, const void* workspace, PoseGraphWs& l, int& n_keys)
{
    if (nodes < 1 || nodes > PG_MAX_NODES || edges < 0 || edges > PG_MAX_EDGES) return false;
    n_keys = 2;
    while (n_keys < 2 * edges) n_keys <<= 1;
    const size_t N = (size_t)nodes, E = (size_t)edges;
    Carver c(workspace, 16);
    l.x_old = c.take<double>(N * 12);
    l.edge_r = c.take<double>(E * 6);
    l.edge_A = c.take<double>(E * PG_EDGE_DOUBLES);
    l.con = c.take<double>(E * 12);
    l.vx = c.take<double>(N * 6);
    l.vr = c.take<double>(N * 6);
    l.vz = c.take<double>(N * 6);
    l.vp = c.take<double>(N * 6);
    l.vq = c.take<double>(N * 6);
    l.hd = c.take<double>(N * 6);
    l.chol = c.take<double>(N * 36);
    l.keys = c.take<unsigned>((size_t)n_keys);
    l.start = c.take<int>(N);
    l.end = c.take<int>(N);
    l.active = c.take<int>(N);
    l.valid = c.take<unsigned char>(E);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_pose_graph_workspace_size(int nodes, int edges)
{
    PoseGraphWs l;
    int n_keys;
    return pose_graph_layout(nodes, edges, nullptr, l, n_keys) ? l.bytes : 0;
}

int gsr_pose_graph_solve(int nodes, int edges, double* poses, const int* fixed, const int* edge_nodes, const double* edge_Z,
                         const double* edge_weights, int outer_iters, int cg_iters, double lambda, double step_tol, float* D, double* stats,
                         void* workspace, size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_pose_graph_solve: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    PoseGraphWs l;
    int n_keys = 0;
    if (nodes < 1 || nodes > PG_MAX_NODES) return fail("nodes must be in [1, 4096], got " + std::to_string(nodes));
    if (edges < 0 || edges > PG_MAX_EDGES) return fail("edges must be in [0, 65536], got " + std::to_string(edges));
    if (outer_iters < 0 || outer_iters > 1000) return fail("outer_iters must be in [0, 1000], got " + std::to_string(outer_iters));
    if (cg_iters < 1 || cg_iters > 100000) return fail("cg_iters must be in [1, 100000], got " + std::to_string(cg_iters));
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail("lambda must be finite and not negative");
    if (!(step_tol >= 0.0) || !std::isfinite(step_tol)) return fail("step_tol must be finite and not negative");
    if (!poses || !fixed || !D || !stats || !workspace) return fail("poses, fixed, D, stats and workspace must not be NULL");
    if (edges > 0 && (!edge_nodes || !edge_Z || !edge_weights)) return fail("edge_nodes, edge_Z and edge_weights must not be NULL when edges > 0");
    pose_graph_layout(nodes, edges, workspace, l, n_keys);
    if (!workspace_fits("gsr_pose_graph_solve", "gsr_pose_graph_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(pose_graph_kernel, dim3(1), dim3(PG_BLOCK), 0, stream, nodes, edges, n_keys, poses, fixed, edge_nodes, edge_Z, edge_weights,
                       outer_iters, cg_iters, lambda, step_tol, D, stats, l);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

int gsr_map_correct(int P, float* xyz, float* rotation, const int* kf_id, int frames, const int* slot_of_frame, int nodes, const float* D,
                    float* quat_workspace, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_map_correct: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    if (P < 0) return fail("P must not be negative, got " + std::to_string(P));
    if (frames < 0) return fail("frames must not be negative, got " + std::to_string(frames));
    if (nodes < 1 || nodes > PG_MAX_NODES) return fail("nodes must be in [1, 4096], got " + std::to_string(nodes));
    if (!D || !quat_workspace) return fail("D and quat_workspace must not be NULL");
    if (frames > 0 && !slot_of_frame) return fail("slot_of_frame must not be NULL when frames > 0");
    if (P > 0 && (!xyz || !rotation || !kf_id)) return fail("xyz, rotation and kf_id must not be NULL when P > 0");
    if (((size_t)xyz | (size_t)rotation | (size_t)kf_id | (size_t)quat_workspace) & 15)
        return fail("xyz, rotation, kf_id and quat_workspace must be 16-byte aligned");
    if (P == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(map_quat_kernel, dim3((unsigned)((nodes + MAPC_BLOCK - 1) / MAPC_BLOCK)), dim3(MAPC_BLOCK), 0, stream, nodes, D, quat_workspace);
    GSR_HIP_CHECK(hipGetLastError());
    const long long groups = ((long long)P + 3) / 4;
    hipLaunchKernelGGL(map_correct_kernel, dim3((unsigned)((groups + MAPC_BLOCK - 1) / MAPC_BLOCK)), dim3(MAPC_BLOCK), 0, stream, P, xyz, rotation,
                       kf_id, frames, slot_of_frame, nodes, D, (const float*)quat_workspace);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_feat_extract: the luma and the corner score of every pixel (bytes) and its 5 x 5 sum (16 bits)
struct FeatExtractLayout { unsigned char* luma; unsigned char* corner; unsigned short* box; size_t bytes; };
static bool feat_extract_layout(int width, int height, const void* workspace, FeatExtractLayout& l)
{
    if (width < 1 || height < 1 || (long long)width * height >= (1LL << 24)) return false;
    const size_t n = (size_t)width * height;
    Carver c(workspace, 16);
    l.luma = c.take<unsigned char>(n);
    l.corner = c.take<unsigned char>(n);
    l.box = c.take<unsigned short>(n);
    l.bytes = c.bytes_padded();
    return true;
}
static int feat_slot_count(int width, int height, int cell, int per_cell)
{
    if (width < 1 || height < 1 || (long long)width * height >= (1LL << 24) || cell < FEAT_MIN_CELL || cell > FEAT_MAX_CELL || per_cell < 1 ||
        per_cell > FEAT_MAX_PER_CELL)
        return 0;
    const long long slots = (long long)((width + cell - 1) / cell) * ((height + cell - 1) / cell) * per_cell;
    return slots <= FEAT_MAX_SLOTS ? (int)slots : 0;
}

int gsr_feat_slots(int width, int height, int cell, int per_cell) { return feat_slot_count(width, height, cell, per_cell); }

size_t gsr_feat_extract_workspace_size(int width, int height)
{
    FeatExtractLayout l;
    return feat_extract_layout(width, height, nullptr, l) ? l.bytes : 0;
}

int gsr_feat_extract(int width, int height, const float* image, const unsigned char* mask, int cell, int per_cell, int threshold,
                     const int* directions, const signed char* pattern, int* keypoints, unsigned int* descriptors, void* workspace,
                     size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_feat_extract: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    FeatExtractLayout l;
    if (!feat_extract_layout(width, height, workspace, l))
        return fail("width and height must be at least 1 and width * height below 2^24, got " + std::to_string(width) + " x " + std::to_string(height));
    if (cell < FEAT_MIN_CELL || cell > FEAT_MAX_CELL) return fail("cell must be in [8, 64], got " + std::to_string(cell));
    if (per_cell < 1 || per_cell > FEAT_MAX_PER_CELL) return fail("per_cell must be in [1, 8], got " + std::to_string(per_cell));
    const int slots = feat_slot_count(width, height, cell, per_cell);
    if (slots < 1) return fail("the frame must have at most 4096 slots (ceil(width / cell) * ceil(height / cell) * per_cell)");
    if (threshold < 0 || threshold > 255) return fail("threshold must be in [0, 255], got " + std::to_string(threshold));
    if (!image || !directions || !pattern || !keypoints || !descriptors || !workspace)
        return fail("image, directions, pattern, keypoints, descriptors and workspace must not be NULL");
    if (!workspace_fits("gsr_feat_extract", "gsr_feat_extract_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const int cells_x = (width + cell - 1) / cell, cells = slots / per_cell;
    hipLaunchKernelGGL(feat_score_kernel, dim3((unsigned)((width + FEAT_TILE - 1) / FEAT_TILE), (unsigned)((height + FEAT_TILE - 1) / FEAT_TILE)),
                       dim3(FEAT_BLOCK), 0, stream, width, height, image, mask, threshold, l.luma, l.corner, l.box);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feat_select_kernel, dim3((unsigned)cells), dim3(FEAT_BLOCK), 0, stream, width, height, cell, per_cell, cells_x,
                       (const unsigned char*)l.corner, keypoints);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feat_describe_kernel, dim3((unsigned)((slots + FEAT_WAVES - 1) / FEAT_WAVES)), dim3(FEAT_BLOCK), 0, stream, width, slots,
                       (const unsigned char*)l.luma, (const unsigned short*)l.box, directions, pattern, keypoints, descriptors);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_feat_match: the best key and the second distance of every slot of A over B, and of every slot of B over A
struct FeatMatchLayout { unsigned* best_ab; int* second_ab; unsigned* best_ba; int* second_ba; size_t bytes; };
static bool feat_slots_ok(int slots) { return slots >= 1 && slots <= FEAT_MAX_SLOTS; }
static bool feat_match_layout(int slots_a, int slots_b, const void* workspace, FeatMatchLayout& l)
{
    if (!feat_slots_ok(slots_a) || !feat_slots_ok(slots_b)) return false;
    Carver c(workspace, 16);
    l.best_ab = c.take<unsigned>((size_t)slots_a);
    l.second_ab = c.take<int>((size_t)slots_a);
    l.best_ba = c.take<unsigned>((size_t)slots_b);
    l.second_ba = c.take<int>((size_t)slots_b);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_feat_match_workspace_size(int slots_a, int slots_b)
{
    FeatMatchLayout l;
    return feat_match_layout(slots_a, slots_b, nullptr, l) ? l.bytes : 0;
}

int gsr_feat_match(int slots_a, const int* keypoints_a, const unsigned int* descriptors_a, int slots_b, const int* keypoints_b,
                   const unsigned int* descriptors_b, int max_distance, int ratio_eighths, int* matches, void* workspace,
                   size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = "gsr_feat_match: " + what; return GSR_ERR_INVALID_ARGUMENT; };
    FeatMatchLayout l;
    if (!feat_match_layout(slots_a, slots_b, workspace, l))
        return fail("slots_a and slots_b must be in [1, 4096], got " + std::to_string(slots_a) + " and " + std::to_string(slots_b));
    if (max_distance < 0 || max_distance > 256) return fail("max_distance must be in [0, 256], got " + std::to_string(max_distance));
    if (ratio_eighths < 0 || ratio_eighths > 8) return fail("ratio_eighths must be in [0, 8], got " + std::to_string(ratio_eighths));
    if (!keypoints_a || !descriptors_a || !keypoints_b || !descriptors_b || !matches || !workspace)
        return fail("keypoints, descriptors, matches and workspace must not be NULL");
    if (!workspace_fits("gsr_feat_match", "gsr_feat_match_workspace_size", workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(feat_nearest_kernel, dim3((unsigned)((slots_a + FEAT_WAVES - 1) / FEAT_WAVES)), dim3(FEAT_BLOCK), 0, stream, slots_a, keypoints_a,
                       descriptors_a, slots_b, keypoints_b, descriptors_b, l.best_ab, l.second_ab);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feat_nearest_kernel, dim3((unsigned)((slots_b + FEAT_WAVES - 1) / FEAT_WAVES)), dim3(FEAT_BLOCK), 0, stream, slots_b, keypoints_b,
                       descriptors_b, slots_a, keypoints_a, descriptors_a, l.best_ba, l.second_ba);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feat_mutual_kernel, dim3((unsigned)((slots_a + FEAT_BLOCK - 1) / FEAT_BLOCK)), dim3(FEAT_BLOCK), 0, stream, slots_a, slots_b,
                       (const unsigned*)l.best_ab, (const int*)l.second_ab, (const unsigned*)l.best_ba, max_distance, ratio_eighths, matches);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace of gsr_feat_pose: the back-projected points of the pair list in both frames, the pixels of B, M, the count of every hypothesis
static bool feat_pose_layout(int slots_a, int hypotheses, const void* workspace, FeatPoseWs& l)
{
    if (!feat_slots_ok(slots_a) || hypotheses < 1 || hypotheses > FEAT_MAX_HYPOTHESES) return false;
    Carver c(workspace, 16);
    l.PA = c.take<float>(3 * (size_t)slots_a);
    l.PB = c.take<float>(3 * (size_t)slots_a);
    l.UV = c.take<float>(2 * (size_t)slots_a);
    l.head = c.take<int>(4);
    l.hyp = c.take<int>((size_t)hypotheses);
    l.bytes = c.bytes_padded();
    return true;
}

size_t gsr_feat_pose_workspace_size(int slots_a, int hypotheses)
{
    FeatPoseWs l;
    return feat_pose_layout(slots_a, hypotheses, nullptr, l) ? l.bytes : 0;
}

// gsr_feat_pose (PNP false) and gsr_feat_pose_pnp (PNP true: depth_b NULL, tau_depth 0): the same checks, workspace and three launches
extern "C++" {
template <bool PNP>
static int feat_pose_run(const char* name, int width, int height, int slots_a, const int* keypoints_a, const float* depth_a, int slots_b,
                         const int* keypoints_b, const float* depth_b, const int* matches, const float* K_a, const float* K_b, unsigned int seed,
                         int hypotheses, float min_area, float tau_px, float tau_depth, int refine_iters, int min_matches, int min_inliers,
                         float min_share, float max_translation, float max_rotation, float* T, int* stats, int* counts, void* workspace,
                         size_t workspace_bytes, void* stream_)
{
    auto fail = [&](const std::string& what) { g_last_error = std::string(name) + ": " + what; return GSR_ERR_INVALID_ARGUMENT; };
    FeatPoseWs l;
    if (width < 1 || height < 1 || (long long)width * height >= 0x80000000LL)
        return fail("width and height must be at least 1 and width * height below 2^31, got " + std::to_string(width) + " x " + std::to_string(height));
    if (!feat_slots_ok(slots_a) || !feat_slots_ok(slots_b))
        return fail("slots_a and slots_b must be in [1, 4096], got " + std::to_string(slots_a) + " and " + std::to_string(slots_b));
    if (!feat_pose_layout(slots_a, hypotheses, workspace, l)) return fail("hypotheses must be in [1, 1024], got " + std::to_string(hypotheses));
    if (!(min_area > 0.f) || !std::isfinite(min_area)) return fail("min_area must be positive and finite");
    if (!(tau_px >= 0.f) || !std::isfinite(tau_px) || !(tau_depth >= 0.f) || !std::isfinite(tau_depth))
        return fail(PNP ? "tau_px must be finite and not negative" : "tau_px and tau_depth must be finite and not negative");
    if (refine_iters < 0 || refine_iters > FEAT_MAX_REFINE) return fail("refine_iters must be in [0, 16], got " + std::to_string(refine_iters));
    if (min_matches < 0) return fail("min_matches must not be negative, got " + std::to_string(min_matches));
    if (min_inliers < 3) return fail("min_inliers must be at least 3, got " + std::to_string(min_inliers));
    if (!(min_share >= 0.f && min_share <= 1.f)) return fail("min_share must be in [0, 1]");
    if (!(max_translation >= 0.f) || !std::isfinite(max_translation) || !(max_rotation >= 0.f) || !std::isfinite(max_rotation))
        return fail("max_translation and max_rotation must be finite and not negative");
    if (!keypoints_a || !depth_a || !keypoints_b || (!PNP && !depth_b) || !matches || !K_a || !K_b || !T || !stats || !workspace)
        return fail(PNP ? "keypoints, depth_a, matches, K_a, K_b, T, stats and workspace must not be NULL"
                        : "keypoints, depths, matches, K_a, K_b, T, stats and workspace must not be NULL");
    const std::string size_name = std::string(name) + "_workspace_size";
    if (!workspace_fits(name, size_name.c_str(), workspace, workspace_bytes, l.bytes)) return GSR_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL((feat_pairs_kernel<PNP>), dim3(1), dim3(FEAT_BLOCK), 0, stream, width, height, slots_a, keypoints_a, depth_a, slots_b,
                       keypoints_b, depth_b, matches, K_a, K_b, l, stats);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((feat_hypotheses_kernel<PNP>), dim3((unsigned)((hypotheses + FEAT_WAVES - 1) / FEAT_WAVES)), dim3(FEAT_BLOCK), 0, stream,
                       hypotheses, seed, min_area, tau_px, tau_depth, K_b, l, counts);
    GSR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((feat_finish_kernel<PNP>), dim3(1), dim3(FEAT_BLOCK), 0, stream, hypotheses, seed, min_area, tau_px, tau_depth, refine_iters,
                       min_matches, min_inliers, min_share, max_translation, max_rotation, K_b, l, T, stats);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // extern "C++"

int gsr_feat_pose(int width, int height, int slots_a, const int* keypoints_a, const float* depth_a, int slots_b, const int* keypoints_b,
                  const float* depth_b, const int* matches, const float* K_a, const float* K_b, unsigned int seed, int hypotheses,
                  float min_area, float tau_px, float tau_depth, int refine_iters, int min_matches, int min_inliers, float min_share,
                  float max_translation, float max_rotation, float* T, int* stats, int* counts, void* workspace, size_t workspace_bytes,
                  void* stream)
{
    return feat_pose_run<false>("gsr_feat_pose", width, height, slots_a, keypoints_a, depth_a, slots_b, keypoints_b, depth_b, matches, K_a, K_b, seed,
                                hypotheses, min_area, tau_px, tau_depth, refine_iters, min_matches, min_inliers, min_share, max_translation,
                                max_rotation, T, stats, counts, workspace, workspace_bytes, stream);
}

// the layout of gsr_feat_pose; PB holds the bearings of B's keypoints
size_t gsr_feat_pose_pnp_workspace_size(int slots_a, int hypotheses) { return gsr_feat_pose_workspace_size(slots_a, hypotheses); }

int gsr_feat_pose_pnp(int width, int height, int slots_a, const int* keypoints_a, const float* depth_a, int slots_b, const int* keypoints_b,
                      const int* matches, const float* K_a, const float* K_b, unsigned int seed, int hypotheses, float min_area, float tau_px,
                      int refine_iters, int min_matches, int min_inliers, float min_share, float max_translation, float max_rotation, float* T,
                      int* stats, int* counts, void* workspace, size_t workspace_bytes, void* stream)
{
    return feat_pose_run<true>("gsr_feat_pose_pnp", width, height, slots_a, keypoints_a, depth_a, slots_b, keypoints_b, nullptr, matches, K_a, K_b,
                               seed, hypotheses, min_area, tau_px, 0.f, refine_iters, min_matches, min_inliers, min_share, max_translation,
                               max_rotation, T, stats, counts, workspace, workspace_bytes, stream);
}

}  // extern "C"
