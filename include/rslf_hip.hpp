// rslf_hip.hpp -- C++11 host side of the MI355X EPI depth scan.
//
// Keeps the constructor / run() shape of rslf::Depth1DComputer_pile<DataType>
// (RSLightFields/include/rslf_depth_computation.hpp:93-143, :425-565) and of
// rslf::Depth1DParameters<DataType> (rslf_depth_computation_core.hpp:66-142) so
// the class drops into the reference's demos (tests/test_depth_computation_pile.cpp:49-51)
// in place of the OpenMP path.  Everything below the class goes through the
// C-ABI of rslf_hip.h; nothing here computes.  The reference's picture getters (get_coloured_epi, get_disparity_map,
// get_coloured_depth_maps) are here too, on byte vectors and a caller's colour table: see "the getters' pictures".
//
// OpenCV is optional: when <opencv2/core/core.hpp> is on the include path
// (the reference's own build, CMakeLists.txt:29) the cv::Mat constructor and
// getters are compiled in; otherwise the same class works on plain pointers.
// Header-only, C++11, exceptions carry the C-ABI's error text.
#ifndef RSLF_HIP_HPP
#define RSLF_HIP_HPP

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rslf_hip.h"

#if defined(__has_include)
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#define RSLFX_HAVE_OPENCV 1
#endif
#endif

namespace rslfx {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& where)
        : std::runtime_error(where + ": " + rslf_status_string(st) + ": " + rslf_last_error()), status(st) {}
};

inline void check(int st, const char* where)
{
    if (st != RSLF_OK)
        throw Error(st, where);
}

// rslf::Depth1DParameters<T>: same member names (par_*), same defaults.
struct Depth1DParameters {
    float par_edge_score_threshold;
    float par_line_score_threshold;
    float par_disp_score_threshold;
    float par_raw_score_threshold;
    float par_mean_shift_max_iter;
    int par_edge_confidence_filter_size;
    int par_edge_confidence_opening_type;
    int par_edge_confidence_opening_size;
    int par_median_filter_size;
    float par_median_filter_epsilon;
    float par_propagation_epsilon;
    float par_slope_factor;
    bool par_cut_shadows;
    float par_shadow_level;
    float par_kernel_bandwidth;   // BandwidthKernel(_BANDWIDTH_KERNEL_PARAMETER), core.hpp:78
    int par_interpolation_class;  // RSLF_INTERP_*: stands for the Interpolation1DClass* of core.hpp:108 (default Linear, :76)
    bool par_use_disp_confidence_score;   // the reference's build switch _USE_DISP_CONFIDENCE_SCORE (core.hpp:35), off by default
    // the reference's build switch _USE_LINE_CONFIDENCE_SCORE (core.hpp:1032-1081) as a mode of Depth2DComputer:
    // RSLF_LINE_CONF_OFF (default) | _AS_BUILT (C_l computed and carried, the gate stays the edge mask) | _GATE (propagation
    // and getters under C_l > par_line_score_threshold).  Host side only: no member of rslf_params.
    int par_line_confidence_mode;

    Depth1DParameters()
    {
        rslf_params p;
        rslf_default_params(&p);
        par_edge_score_threshold = p.edge_score_threshold;
        par_line_score_threshold = p.line_score_threshold;
        par_disp_score_threshold = p.disp_score_threshold;
        par_raw_score_threshold = p.raw_score_threshold;
        par_mean_shift_max_iter = p.mean_shift_max_iter;
        par_edge_confidence_filter_size = p.edge_confidence_filter_size;
        par_edge_confidence_opening_type = p.edge_confidence_opening_type;
        par_edge_confidence_opening_size = p.edge_confidence_opening_size;
        par_median_filter_size = p.median_filter_size;
        par_median_filter_epsilon = p.median_filter_epsilon;
        par_propagation_epsilon = p.propagation_epsilon;
        par_slope_factor = p.slope_factor;
        par_cut_shadows = p.cut_shadows != 0;
        par_shadow_level = p.shadow_level;
        par_kernel_bandwidth = p.kernel_bandwidth;
        par_interpolation_class = p.interpolation;
        par_use_disp_confidence_score = p.use_disp_confidence_score != 0;
        par_line_confidence_mode = RSLF_LINE_CONF_OFF;
    }

    static Depth1DParameters& get_default()
    {
        static Depth1DParameters s_default;   // core.hpp:138-142
        return s_default;
    }

    rslf_params to_c() const
    {
        rslf_params p;
        p.edge_score_threshold = par_edge_score_threshold;
        p.line_score_threshold = par_line_score_threshold;
        p.disp_score_threshold = par_disp_score_threshold;
        p.raw_score_threshold = par_raw_score_threshold;
        p.mean_shift_max_iter = par_mean_shift_max_iter;
        p.edge_confidence_filter_size = par_edge_confidence_filter_size;
        p.edge_confidence_opening_type = par_edge_confidence_opening_type;
        p.edge_confidence_opening_size = par_edge_confidence_opening_size;
        p.median_filter_size = par_median_filter_size;
        p.median_filter_epsilon = par_median_filter_epsilon;
        p.propagation_epsilon = par_propagation_epsilon;
        p.slope_factor = par_slope_factor;
        p.cut_shadows = par_cut_shadows ? 1 : 0;
        p.shadow_level = par_shadow_level;
        p.kernel_bandwidth = par_kernel_bandwidth;
        p.interpolation = par_interpolation_class;
        p.use_disp_confidence_score = par_use_disp_confidence_score ? 1 : 0;
        return p;
    }
};

// The element type of a host light field: the cv::Mat depths the reference's constructors take (CV_32F, CV_8U and, as every
// depth other than 8U, CV_16U: dc.hpp:269-288, :442-475, :671-705).  U8 is normalised by 1/255; F32 and U16 by the max over
// all values, or by epi_scale_factor when it is >= 0 -- a U16 field gives the slab of the same values given as float.
enum class InputType { F32, U8, U16 };

namespace detail {

// the constructor's copy (dc.hpp:425-477) into vol; returns the epi_scale_factor used
inline float upload_epis(rslf_volume* vol, InputType type, const void* const* epis, size_t row_stride_bytes, float epi_scale_factor)
{
    float used = 255.f;
    switch (type) {
    case InputType::U8:
        check(rslf_volume_upload_epis_u8(vol, (const uint8_t* const*)epis, row_stride_bytes), "rslf_volume_upload_epis_u8");
        break;
    case InputType::U16:
        check(rslf_volume_upload_epis_u16(vol, (const uint16_t* const*)epis, row_stride_bytes, epi_scale_factor, &used),
              "rslf_volume_upload_epis_u16");
        break;
    default:
        check(rslf_volume_upload_epis_f32(vol, (const float* const*)epis, row_stride_bytes, epi_scale_factor, &used),
              "rslf_volume_upload_epis_f32");
    }
    return used;
}

// ---- the getters' pictures ------------------------------------------------------------------------------------------
// The classes below hold their results on the host, so their getters go through the host-pointer forms of the renderers
// (rslf_render_planes_host, rslf_render_epi_lines_host).  Pictures are dense uint8 BGR vectors; `lut_bgr` is the caller's
// table of 256 x 3 bytes (level i -> lut_bgr[3 i .. 3 i + 2]), which stands where the reference takes a cv colormap id.
// The rules (index defaults, masks, fits, formulas) are those of remotesensingproject_amd/depth.py's getters, which cite
// the reference line by line; where the reference's own index runs past the end, the getter throws
// Error(RSLF_ERR_INVALID_ARG).  Each getter has a form whose first argument is the Context to render on: an object
// built on a MultiContext has no context of its own (rendering OVER several devices is not built).

inline void require(bool ok, const char* what)
{
    if (!ok) {
        rslf_render_centre_index(0, nullptr);   // sets the library's error text to "bad arguments"
        throw Error(RSLF_ERR_INVALID_ARG, what);
    }
}

// fit (fit_plane = -1: every plane its own range; k: plane k's range for all) + render of host planes -> [n][rows][cols][3]
inline std::vector<uint8_t> render_planes(rslf_ctx* ctx, const std::vector<float>& planes, size_t offset, const uint8_t* valid, int n,
                                          size_t plane_stride, int rows, int cols, size_t row_stride, int fit_mode, int fit_plane,
                                          int formula, const uint8_t* lut_bgr, const rslf_volume* vol = nullptr, float shadow_level = 0.f)
{
    require(!planes.empty(), "the getters show the results of run(): call it first");
    std::vector<uint8_t> out((size_t)n * rows * cols * 3);
    check(rslf_render_planes_host(ctx, planes.data() + offset, n, plane_stride, rows, cols, row_stride, valid ? valid + offset : nullptr,
                                  fit_mode, fit_plane, 0, formula, lut_bgr, RSLF_MASK_BLACK, vol, RSLF_SLICE_VIEW, 0, shadow_level,
                                  out.data(), nullptr),
          "rslf_render_planes_host");
    return out;
}

#ifdef RSLFX_HAVE_OPENCV
// The data pointers of a Vec<Mat> of EPIs and their element type; one shape, one row step (the library takes ONE
// row_stride_bytes for all: a clone among ROI Mats is refused, not misread), one type, `channels` channels.  CV_16U is
// accepted where the OpenCV in use defines it (a macro in every OpenCV release).
inline std::vector<const void*> mat_pointers(const std::vector<cv::Mat>& epis, int channels, InputType& type, const char* who)
{
    if (epis.empty())
        throw std::invalid_argument(std::string(who) + ": no EPIs");
    if (epis[0].channels() != channels)
        throw std::invalid_argument(std::string(who) + ": channel count does not match the instantiation");
    std::vector<const void*> ptrs(epis.size());
    for (size_t v = 0; v < epis.size(); v++) {
        if (epis[v].rows != epis[0].rows || epis[v].cols != epis[0].cols || epis[v].type() != epis[0].type())
            throw std::invalid_argument(std::string(who) + ": EPIs differ in size or type");
        if (epis[v].step[0] != epis[0].step[0])
            throw std::invalid_argument(std::string(who) + ": EPIs differ in their row step (clone() the ROI Mats, or none)");
        ptrs[v] = epis[v].data;
    }
    const int depth = epis[0].depth();
    if (depth == CV_8U)
        type = InputType::U8;
    else if (depth == CV_32F)
        type = InputType::F32;
#ifdef CV_16U
    else if (depth == CV_16U)
        type = InputType::U16;
    else
        throw std::invalid_argument(std::string(who) + ": EPIs must be CV_8U, CV_16U or CV_32F");
#else
    else
        throw std::invalid_argument(std::string(who) + ": EPIs must be CV_8U or CV_32F");
#endif
    return ptrs;
}

// A Vec<Mat> as the pointer constructors take it
struct MatInput {
    std::vector<const void*> ptrs;
    InputType type;
    int V, S, U;
    size_t stride;
    MatInput(const std::vector<cv::Mat>& epis, int channels, const char* who) : type(InputType::F32)
    {
        ptrs = mat_pointers(epis, channels, type, who);
        V = (int)epis.size();
        S = epis[0].rows;
        U = epis[0].cols;
        stride = epis[0].step[0];
    }
};
#endif

}  // namespace detail

// RAII handles
class Context {
public:
    explicit Context(int device = 0) : h_(nullptr) { check(rslf_ctx_create(device, &h_), "rslf_ctx_create"); }
    ~Context() { rslf_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    rslf_ctx* get() const { return h_; }
    void set_stream(void* hip_stream) { check(rslf_ctx_set_stream(h_, hip_stream), "rslf_ctx_set_stream"); }
    void synchronize() { check(rslf_ctx_synchronize(h_), "rslf_ctx_synchronize"); }
    float last_scan_kernel_ms()
    {
        float ms = 0;
        check(rslf_last_scan_kernel_ms(h_, &ms), "rslf_last_scan_kernel_ms");
        return ms;
    }

private:
    rslf_ctx* h_;
};

namespace detail {
inline Context& own(Context* ctx)   // the context an object was built on
{
    if (!ctx)
        throw std::invalid_argument("this object was built on a MultiContext: pass the Context to render on");
    return *ctx;
}

// Not in the reference: the dilation along u (rslf_volume_dilate_u, rslf_hip.h) as the computers' set_u_dilation holds it --
// the volume as it was uploaded, its width and the caller's slope factor, and the factor in force.
struct Dilation {
    rslf_volume* source;
    int dim_u, factor;
    float slope;
    Dilation() : source(nullptr), dim_u(0), factor(1), slope(1.f) {}
};
// The computer's volume, width and slope factor (its members, by reference) put into the frame of `factor`: the volume
// dilated from the source on the device, U' = factor * (U - 1) + 1 columns, slope factor float(source's) * float(factor).
// Factor 1 puts the source back; nothing is launched or allocated for it.
inline void set_u_dilation(Dilation& d, Context* ctx, rslf_volume*& vol, int& dim_u, float& slope, int factor, int kind)
{
    if (!ctx)
        throw std::invalid_argument("set_u_dilation: this object was built on a MultiContext: the dilation along u is built for one context");
    if (!d.source) {
        d.source = vol;
        d.dim_u = dim_u;
        d.slope = slope;
    }
    int wide = 0;
    check(rslf_dilated_width(d.dim_u, factor, &wide), "rslf_dilated_width");
    require(kind == RSLF_DILATE_LINEAR || kind == RSLF_DILATE_CUBIC || kind == RSLF_DILATE_LANCZOS3,
            "set_u_dilation: RSLF_DILATE_LINEAR, RSLF_DILATE_CUBIC or RSLF_DILATE_LANCZOS3");
    rslf_volume* next = nullptr;
    if (factor != 1)
        check(rslf_volume_dilate_u(ctx->get(), d.source, factor, kind, &next), "rslf_volume_dilate_u");
    else
        next = d.source;
    if (vol != d.source)
        rslf_volume_destroy(vol);
    vol = next;
    dim_u = wide;
    slope = d.slope * (float)factor;
    d.factor = factor;
}
// planes[rows][U'] of the dilated frame on the source grid, [rows][U] (rslf_planes_undilate_u_host).
template <typename T>
inline std::vector<T> undilated(const std::vector<T>& planes, int dim_u, int factor)
{
    require(!planes.empty(), "the getters show the results of run(): call it first");
    const size_t rows = planes.size() / (size_t)dim_u;
    std::vector<T> out(rows * (size_t)((dim_u - 1) / factor + 1));
    check(rslf_planes_undilate_u_host(planes.data(), 0, (int)sizeof(T), rows, dim_u, factor, out.data(), 0), "rslf_planes_undilate_u_host");
    return out;
}
}  // namespace detail

// Several devices (or several workers on one device) behind one handle: the pile path then cuts the scanlines into one
// block per device and overlaps upload, kernels and download chunk by chunk (rslf_hip.h, rslf_multi_*).
// Not in the reference: the result of the cross-view consistency check (rslf_view_consistency, rslf_hip.h), [S][V][U] each
// -- per pixel the other views in field (seen), those whose pixel on the pixel's EPI line is valid and within tol (agree),
// more than tol above, more than tol below; fused, the mean of the pixel's disparity and the agreeing ones; valid, 255
// where agree >= min_agree.  What above and below mean depends on the field's sign convention (rslf_hip.h).
struct Consistency {
    std::vector<int32_t> seen, agree, above, below;
    std::vector<float> fused;
    std::vector<uint8_t> valid;
};

namespace detail {
// n cells each, and the C struct of the four count planes
inline rslf_view_counts consistency_planes(Consistency& c, size_t n)
{
    c.seen.resize(n), c.agree.resize(n), c.above.resize(n), c.below.resize(n), c.fused.resize(n), c.valid.resize(n);
    const rslf_view_counts counts = {c.seen.data(), c.agree.data(), c.above.data(), c.below.data()};
    return counts;
}
// the getters' default tolerance: one step of the hypothesis grid
inline float grid_step(float dmin, float dmax, int dim_d)
{
    require(dim_d >= 2, "get_consistency: one hypothesis has no grid step: pass tol");
    return (float)(((double)dmax - (double)dmin) / (dim_d - 1));
}
}  // namespace detail

// Not in the reference: the planes of the view warp (rslf_view_warp, rslf_hip.h) for the T targets of a call, [T][V][U] each
// (colour [T][V][U][C]) -- hit 255 where a source pixel arrived; depth, src_view, src_col the winner's stored disparity, view
// and column (0, -1, -1 where none); count the candidates that arrived; colour the light field's radiance at the winner.
struct Warp {
    std::vector<uint8_t> hit;
    std::vector<float> depth;
    std::vector<int32_t> src_view, src_col, count;
    std::vector<float> colour;
};
// ... and the leave-one-out yardstick: every target view predicted from the OTHER views and compared with the view that was
// taken -- err and hit [T][V][U], row_err / row_hits [T][V], and per target mean_abs_error (NaN where nothing arrived) and
// coverage (hits over V * U).
struct ViewPrediction {
    std::vector<float> err;
    std::vector<uint8_t> hit;
    std::vector<double> row_err;
    std::vector<int32_t> row_hits;
    std::vector<double> mean_abs_error, coverage;
};

// Not in the reference: the planes of the novel view (rslf_novel_view, rslf_hip.h) of one target, [V][U] each (colour
// [V][U][C]) -- fill 0 hole / 1 hit / 2, 3 filled from the left / right bound; depth the disparity of every target pixel (0 at
// holes); n_src the views blended; colour the finished image (empty when not asked for).
struct NovelView {
    std::vector<float> colour, depth;
    std::vector<uint8_t> fill;
    std::vector<int32_t> n_src;
};
// What a novel view is made with: radius, nearer as the warp's; max_gap > 0: runs of more columns stay holes; sources: the
// views blended at most; tol < 0: one step of the hypothesis grid.
struct NovelViewOptions {
    int radius = 0, nearer = 1, max_gap = 0, sources = 4;
    float tol = -1.f;
};

namespace detail {
inline rslf_novel_view_out novel_planes(NovelView& w, size_t n, int channels, bool colour)
{
    w.depth.resize(n), w.fill.resize(n), w.n_src.resize(n);
    if (colour)
        w.colour.resize(n * (size_t)channels);
    const rslf_novel_view_out out = {colour ? w.colour.data() : nullptr, w.depth.data(), w.fill.data(), w.n_src.data(), nullptr, nullptr, nullptr};
    return out;
}
inline rslf_novel_view_params novel_params(const NovelViewOptions& o, float step)
{
    const rslf_novel_view_params p = {o.radius, o.nearer, o.max_gap, o.sources, o.tol < 0.f ? step : o.tol};
    return p;
}
inline rslf_view_warp_out warp_planes(Warp& w, size_t n, int channels, bool colour)
{
    w.hit.resize(n), w.depth.resize(n), w.src_view.resize(n), w.src_col.resize(n), w.count.resize(n);
    if (colour)
        w.colour.resize(n * (size_t)channels);
    const rslf_view_warp_out out = {w.hit.data(), w.depth.data(), w.src_view.data(), w.src_col.data(), w.count.data(),
                                    colour ? w.colour.data() : nullptr, nullptr, nullptr, nullptr};
    return out;
}
inline rslf_view_warp_out prediction_planes(ViewPrediction& p, int T, int V, int U)
{
    p.err.resize((size_t)T * V * U), p.hit.resize((size_t)T * V * U), p.row_err.resize((size_t)T * V), p.row_hits.resize((size_t)T * V);
    const rslf_view_warp_out out = {p.hit.data(), nullptr, nullptr, nullptr, nullptr, nullptr, p.err.data(), p.row_err.data(), p.row_hits.data()};
    return out;
}
inline void prediction_finish(ViewPrediction& p, int T, int V, int U)
{
    p.mean_abs_error.assign((size_t)T, std::nan("")), p.coverage.assign((size_t)T, 0.0);
    for (int k = 0; k < T; k++) {
        double e = 0.0;
        long long hits = 0;
        for (int v = 0; v < V; v++)
            e += p.row_err[(size_t)k * V + v], hits += p.row_hits[(size_t)k * V + v];
        if (hits)
            p.mean_abs_error[(size_t)k] = e / (double)hits;
        p.coverage[(size_t)k] = (double)hits / ((double)V * U);
    }
}
// the default targets of a prediction: every view, each excluded from its own
inline std::vector<float> prediction_targets(std::vector<int>& views, int S)
{
    if (views.empty())
        for (int s = 0; s < S; s++)
            views.push_back(s);
    return std::vector<float>(views.begin(), views.end());
}
}  // namespace detail

class MultiContext {
public:
    MultiContext() : h_(nullptr) { check(rslf_multi_create(nullptr, 0, &h_), "rslf_multi_create"); }
    explicit MultiContext(const std::vector<int>& devices) : h_(nullptr)
    {
        check(rslf_multi_create(devices.empty() ? nullptr : devices.data(), (int)devices.size(), &h_), "rslf_multi_create");
    }
    ~MultiContext() { rslf_multi_destroy(h_); }
    MultiContext(const MultiContext&) = delete;
    MultiContext& operator=(const MultiContext&) = delete;
    rslf_multi* get() const { return h_; }
    int device_count() const { return rslf_multi_device_count(h_); }
    void set_chunk_rows(int rows) { check(rslf_multi_set_chunk_rows(h_, rows), "rslf_multi_set_chunk_rows"); }

private:
    rslf_multi* h_;
};

// rslf::Depth1DComputer_pile<DataType>.  DataType is float (1 channel) or a
// 3-float pixel (cv::Vec3f in the reference, dc.hpp:149-154): only its channel
// count matters here.
template <int CHANNELS>
class Depth1DComputer_pile {
public:
    // The reference's constructor (dc.hpp:97-106) on raw pointers: epis[v] points
    // at an S x U image of CHANNELS interleaved values, rows row_stride_bytes
    // apart (cv::Mat::data / cv::Mat::step; 0 = dense).  is_u8 selects the
    // uchar branch of dc.hpp:468-475.
    Depth1DComputer_pile(Context& ctx, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u,
                         size_t row_stride_bytes, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(&ctx), multi_(nullptr), vol_(nullptr), m_parameters(parameters)
    {
        init(epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d, s_hat,
             epi_scale_factor);
    }
    // The same with the element type named (InputType::U16: CV_16U EPIs, normalised like float).
    Depth1DComputer_pile(Context& ctx, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u,
                         size_t row_stride_bytes, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(&ctx), multi_(nullptr), vol_(nullptr), m_parameters(parameters)
    {
        init(epis, type, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d, s_hat, epi_scale_factor);
    }

    // The same on a MultiContext: the scanlines are shared out over its devices and the host copies overlap the kernels.
    // Here the EPIs are read by run(), not copied by the constructor: the buffers must outlive it (they do in the
    // reference's demos, where the Vec<Mat> lives next to the computer).
    Depth1DComputer_pile(MultiContext& multi, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u,
                         size_t row_stride_bytes, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(nullptr), multi_(&multi), vol_(nullptr), m_parameters(parameters)
    {
        init_multi(epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d, s_hat,
                   epi_scale_factor);
    }
    Depth1DComputer_pile(MultiContext& multi, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u,
                         size_t row_stride_bytes, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(nullptr), multi_(&multi), vol_(nullptr), m_parameters(parameters)
    {
        init_multi(epis, type, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d, s_hat, epi_scale_factor);
    }

#ifdef RSLFX_HAVE_OPENCV
    Depth1DComputer_pile(MultiContext& multi, const std::vector<cv::Mat>& epis, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(nullptr), multi_(&multi), vol_(nullptr), m_parameters(parameters)
    {
        InputType type = InputType::F32;
        const std::vector<const void*> ptrs = mat_pointers(epis, type);
        init_multi(ptrs.data(), type, (int)epis.size(), epis[0].rows, epis[0].cols, epis[0].step[0], dmin, dmax, dim_d, s_hat,
                   epi_scale_factor);
    }
    // Exactly the reference's signature: Vec<Mat> in (dc.hpp:97-106).
    Depth1DComputer_pile(Context& ctx, const std::vector<cv::Mat>& epis, float dmin, float dmax, int dim_d, int s_hat = -1,
                         float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(&ctx), multi_(nullptr), vol_(nullptr), m_parameters(parameters)
    {
        InputType type = InputType::F32;
        const std::vector<const void*> ptrs = mat_pointers(epis, type);
        init(ptrs.data(), type, (int)epis.size(), epis[0].rows, epis[0].cols, epis[0].step[0], dmin, dmax, dim_d, s_hat,
             epi_scale_factor);
    }
    static std::vector<const void*> mat_pointers(const std::vector<cv::Mat>& epis, InputType& type)
    {
        return detail::mat_pointers(epis, CHANNELS, type, "Depth1DComputer_pile");
    }
    // (the two-type form: CV_8U or CV_32F)
    static std::vector<const void*> mat_pointers(const std::vector<cv::Mat>& epis, bool& is_u8)
    {
        InputType type = InputType::F32;
        std::vector<const void*> ptrs = mat_pointers(epis, type);
        if (type == InputType::U16)
            throw std::invalid_argument("Depth1DComputer_pile: CV_16U EPIs need the InputType form of mat_pointers");
        is_u8 = type == InputType::U8;
        return ptrs;
    }
    cv::Mat get_edge_confidence() const { return cv::Mat(dim_v_, dim_u_, CV_32FC1, (void*)m_edge_confidence_v_u.data()).clone(); }
    cv::Mat get_edge_confidence_mask() const { return cv::Mat(dim_v_, dim_u_, CV_8UC1, (void*)m_edge_confidence_mask_v_u.data()).clone(); }
    cv::Mat get_disp_confidence() const { return cv::Mat(dim_v_, dim_u_, CV_32FC1, (void*)m_disp_confidence_v_u.data()).clone(); }
    cv::Mat get_best_depth() const { return cv::Mat(dim_v_, dim_u_, CV_32FC1, (void*)m_best_depth_v_u.data()).clone(); }
    cv::Mat get_rbar() const { return cv::Mat(dim_v_, dim_u_, CV_32FC(CHANNELS), (void*)m_rbar_v_u.data()).clone(); }
#endif

    ~Depth1DComputer_pile()
    {
        rslf_volume_destroy(vol_);
        if (dilation_.source != vol_)
            rslf_volume_destroy(dilation_.source);
    }
    Depth1DComputer_pile(const Depth1DComputer_pile&) = delete;
    Depth1DComputer_pile& operator=(const Depth1DComputer_pile&) = delete;

    // dc.hpp:513-565: edge confidence, scan, selective median -- on the GPU -- then the
    // result planes are copied into the host members below.
    void run()
    {
        const size_t n = (size_t)dim_v_ * dim_u_;
        m_edge_confidence_v_u.assign(n, 0.f);
        m_edge_confidence_mask_v_u.assign(n, 0);
        m_disp_confidence_v_u.assign(n, 0.f);
        m_best_depth_v_u.assign(n, 0.f);
        m_rbar_v_u.assign(n * CHANNELS, 0.f);
        m_depth_idx_v_u.assign(n, -1);
        m_score_v_u.assign(n, 0.f);
        const rslf_params p = m_parameters.to_c();
        if (multi_) {
            if (type_ == InputType::U8)
                check(rslf_multi_depth1d_pile_u8(multi_->get(), (const uint8_t* const*)epis_.data(), row_stride_bytes_, dim_v_, dim_s_,
                                                 dim_u_, CHANNELS, m_dmin, m_dmax, m_dim_d, m_s_hat, &p, m_edge_confidence_v_u.data(),
                                                 m_edge_confidence_mask_v_u.data(), m_disp_confidence_v_u.data(),
                                                 m_best_depth_v_u.data(), m_rbar_v_u.data(), m_depth_idx_v_u.data(),
                                                 m_score_v_u.data(), nullptr, &stats),
                      "rslf_multi_depth1d_pile_u8");
            else if (type_ == InputType::U16)
                check(rslf_multi_depth1d_pile_u16(multi_->get(), (const uint16_t* const*)epis_.data(), row_stride_bytes_, dim_v_, dim_s_,
                                                  dim_u_, CHANNELS, epi_scale_arg_, m_dmin, m_dmax, m_dim_d, m_s_hat, &p,
                                                  m_edge_confidence_v_u.data(), m_edge_confidence_mask_v_u.data(),
                                                  m_disp_confidence_v_u.data(), m_best_depth_v_u.data(), m_rbar_v_u.data(),
                                                  m_depth_idx_v_u.data(), m_score_v_u.data(), nullptr, &stats, &scale_used_),
                      "rslf_multi_depth1d_pile_u16");
            else
                check(rslf_multi_depth1d_pile_f32(multi_->get(), (const float* const*)epis_.data(), row_stride_bytes_, dim_v_, dim_s_,
                                                  dim_u_, CHANNELS, epi_scale_arg_, m_dmin, m_dmax, m_dim_d, m_s_hat, &p,
                                                  m_edge_confidence_v_u.data(), m_edge_confidence_mask_v_u.data(),
                                                  m_disp_confidence_v_u.data(), m_best_depth_v_u.data(), m_rbar_v_u.data(),
                                                  m_depth_idx_v_u.data(), m_score_v_u.data(), nullptr, &stats, &scale_used_),
                      "rslf_multi_depth1d_pile_f32");
            return;
        }
        // (subgrid 0: exactly rslf_depth1d_pile_run_host's launches and planes)
        check(rslf_depth1d_pile_run_host_sub(ctx_->get(), vol_, m_dmin, m_dmax, m_dim_d, m_s_hat, &p, m_edge_confidence_v_u.data(),
                                             m_edge_confidence_mask_v_u.data(), m_disp_confidence_v_u.data(),
                                             m_best_depth_v_u.data(), m_rbar_v_u.data(), m_depth_idx_v_u.data(),
                                             m_score_v_u.data(), nullptr, &stats, subgrid_ ? 1 : 0),
              "rslf_depth1d_pile_run_host_sub");
    }

    // Not in the reference: with the mode on, run() moves every disparity the scan assigns off the hypothesis grid -- the
    // vertex of the parabola through the winner's score and its two neighbours', within half a grid step
    // (rslf_subgrid_refine, rslf_hip.h) -- before the selective median filters the plane; m_best_depth_v_u and the pictures
    // of the getters then hold refined values, every other member is unchanged.  Default off.  One context: an object built
    // on a MultiContext throws with the mode on, as get_peaks does.
    void set_subgrid(bool on)
    {
        if (on && multi_)
            throw std::invalid_argument("set_subgrid: this object was built on a MultiContext: the sub-grid mode is built for one context");
        subgrid_ = on;
    }
    bool get_subgrid() const { return subgrid_; }

    // Not in the reference's code (its report's fourth lead), to be called before run(): the EPIs are resampled along u on the
    // device by the integer `factor` (1..8) with the kernel `kind` (RSLF_DILATE_*; rslf_volume_dilate_u, rslf_hip.h), and the
    // object then behaves bit for bit as if built from the dilated EPIs with par_slope_factor * factor: every member and
    // getter answers in the dilated frame, u_dilated() = factor * (dim_u - 1) + 1 columns wide (cols() too).  The results of
    // an earlier run() are dropped.  Factor 1 puts the source back.  One context: throws on a MultiContext.
    void set_u_dilation(int factor, int kind = RSLF_DILATE_CUBIC)
    {
        detail::set_u_dilation(dilation_, multi_ ? nullptr : ctx_, vol_, dim_u_, m_parameters.par_slope_factor, factor, kind);
        m_edge_confidence_v_u.clear(), m_edge_confidence_mask_v_u.clear(), m_disp_confidence_v_u.clear(), m_best_depth_v_u.clear();
        m_rbar_v_u.clear(), m_depth_idx_v_u.clear(), m_score_v_u.clear();
    }
    int get_u_dilation() const { return dilation_.factor; }
    int u_dilated() const { return dim_u_; }
    // m_best_depth_v_u and m_edge_confidence_mask_v_u on the source grid, [V][U]: their columns u * factor.
    std::vector<float> get_best_depth_undilated() const { return detail::undilated(m_best_depth_v_u, dim_u_, dilation_.factor); }
    std::vector<uint8_t> get_edge_confidence_mask_undilated() const
    {
        return detail::undilated(m_edge_confidence_mask_v_u, dim_u_, dilation_.factor);
    }

    int get_s_hat() const { return m_s_hat; }

    // dc.hpp:568-617: the EPI of scanline a_v (< 0: floor(V / 2.0)) with every confident pixel's line drawn in the colour
    // of its disparity, nearer lines over farther ones -> [S][U][3].  The loop's sequential meaning (under OpenMP the
    // reference's loop races).
    std::vector<uint8_t> get_coloured_epi(Context& on, int a_v, const uint8_t* lut_bgr) const
    {
        detail::require(!m_best_depth_v_u.empty(), "the getters show the results of run(): call it first");
        if (a_v < 0)
            a_v = (int)std::floor(dim_v_ / 2.0);   // :576-577
        detail::require(a_v < dim_v_, "get_coloured_epi: the scanline is not below dim_v");
        std::vector<uint8_t> out((size_t)dim_s_ * dim_u_ * 3);
        check(rslf_render_epi_lines_host(on.get(), m_best_depth_v_u.data(), m_edge_confidence_mask_v_u.data(), dim_v_, dim_s_, dim_u_, m_s_hat,
                                         a_v, 1, lut_bgr, out.data()),
              "rslf_render_epi_lines_host");
        return out;
    }
    std::vector<uint8_t> get_coloured_epi(int a_v, const uint8_t* lut_bgr) const { return get_coloured_epi(detail::own(ctx_), a_v, lut_bgr); }
    // dc.hpp:619-643: the disparities scaled over their min / max (every pixel, confident or not), colour-mapped, black
    // outside m_edge_confidence_mask_v_u -> [V][U][3]
    std::vector<uint8_t> get_disparity_map(Context& on, const uint8_t* lut_bgr) const
    {
        return detail::render_planes(on.get(), m_best_depth_v_u, 0, m_edge_confidence_mask_v_u.data(), 1, 0, dim_v_, dim_u_, (size_t)dim_u_,
                                     RSLF_FIT_MINMAX, -1, RSLF_RENDER_SHIFT, lut_bgr);
    }
    std::vector<uint8_t> get_disparity_map(const uint8_t* lut_bgr) const { return get_disparity_map(detail::own(ctx_), lut_bgr); }

    // After run(): the score rows [n_rows][U][dim_d] of scanlines [v_first, v_first + n_rows) (n_rows < 0: to the last
    // one), the reference's buf_scores_u_d of each EPI (core.hpp:616-625), over the pixels of the final edge-confidence
    // mask -- those that received a disparity; the rows of every other pixel are 0.  A scan of its own on the object's
    // context.  An object built on a MultiContext keeps no volume on a device: it refuses.
    std::vector<float> get_scores(int v_first = 0, int n_rows = -1) const
    {
        if (multi_)
            throw std::invalid_argument("get_scores: this object was built on a MultiContext, which keeps no volume on a device: "
                                        "score rows are built for one context");
        detail::require(!m_best_depth_v_u.empty(), "the getters show the results of run(): call it first");
        if (n_rows < 0)
            n_rows = dim_v_ - v_first;
        detail::require(v_first >= 0 && n_rows > 0 && n_rows <= dim_v_ - v_first, "get_scores: the scanlines are not a window of the volume");
        std::vector<float> out((size_t)n_rows * dim_u_ * m_dim_d);
        const rslf_params p = m_parameters.to_c();
        check(rslf_depth_epi_scores_host(ctx_->get(), vol_, nullptr, nullptr, m_dmin, m_dmax, m_dim_d, m_s_hat, &p,
                                         m_edge_confidence_mask_v_u.data(), v_first, n_rows, out.data(), nullptr),
              "rslf_depth_epi_scores_host");
        return out;
    }

    // After run(): the peaks of those score rows (rslf_hip.h, rslf_peaks) -- winner, sub-grid disparity, runner-up -- over
    // the pixels of the final edge-confidence mask, [n_rows][U] each; other pixels hold -1 / 0.  The rows stay on the
    // device.  Refused on a MultiContext, as get_scores is.
    struct Peaks {
        std::vector<int32_t> idx, runner_idx;
        std::vector<float> score, disp, runner_score;
    };
    Peaks get_peaks(int v_first = 0, int n_rows = -1) const
    {
        if (multi_)
            throw std::invalid_argument("get_peaks: this object was built on a MultiContext, which keeps no volume on a device: "
                                        "score-row peaks are built for one context");
        detail::require(!m_best_depth_v_u.empty(), "the getters show the results of run(): call it first");
        if (n_rows < 0)
            n_rows = dim_v_ - v_first;
        detail::require(v_first >= 0 && n_rows > 0 && n_rows <= dim_v_ - v_first, "get_peaks: the scanlines are not a window of the volume");
        const size_t n = (size_t)n_rows * dim_u_;
        Peaks out;
        out.idx.resize(n), out.runner_idx.resize(n), out.score.resize(n), out.disp.resize(n), out.runner_score.resize(n);
        const rslf_peaks planes = {out.idx.data(), out.score.data(), out.disp.data(), out.runner_idx.data(), out.runner_score.data()};
        const rslf_params p = m_parameters.to_c();
        check(rslf_depth_epi_peaks_host(ctx_->get(), vol_, nullptr, nullptr, m_dmin, m_dmax, m_dim_d, m_s_hat, &p,
                                        m_edge_confidence_mask_v_u.data(), v_first, n_rows, &planes, nullptr),
              "rslf_depth_epi_peaks_host");
        return out;
    }

    int rows() const { return dim_v_; }
    int cols() const { return dim_u_; }
    float epi_scale_factor() const { return scale_used_; }

    // Results, dense row-major [V][U] (what the reference keeps as private Mats, dc.hpp:131-135)
    std::vector<float> m_edge_confidence_v_u;
    std::vector<uint8_t> m_edge_confidence_mask_v_u;
    std::vector<float> m_disp_confidence_v_u;
    std::vector<float> m_best_depth_v_u;
    std::vector<float> m_rbar_v_u;          // [V][U][CHANNELS]
    std::vector<int32_t> m_depth_idx_v_u;   // argmax index, -1 where no disparity was assigned
    std::vector<float> m_score_v_u;
    rslf_stats stats;

private:
    void init(const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes, float dmin,
              float dmax, int dim_d, int s_hat, float epi_scale_factor)
    {
        dim_v_ = dim_v;
        dim_s_ = dim_s;
        dim_u_ = dim_u;
        m_dmin = dmin;
        m_dmax = dmax;
        m_dim_d = dim_d;
        // dc.hpp:490-498
        m_s_hat = (s_hat < 0 || s_hat > dim_s - 1) ? (int)std::floor((0.0 + dim_s) / 2) : s_hat;
        stats = rslf_stats();
        check(rslf_volume_create(ctx_->get(), dim_v, dim_s, dim_u, CHANNELS, &vol_), "rslf_volume_create");
        type_ = type;
        scale_used_ = detail::upload_epis(vol_, type, epis, row_stride_bytes, epi_scale_factor);
    }
    void init_multi(const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes, float dmin,
                    float dmax, int dim_d, int s_hat, float epi_scale_factor)
    {
        dim_v_ = dim_v;
        dim_s_ = dim_s;
        dim_u_ = dim_u;
        m_dmin = dmin;
        m_dmax = dmax;
        m_dim_d = dim_d;
        m_s_hat = (s_hat < 0 || s_hat > dim_s - 1) ? (int)std::floor((0.0 + dim_s) / 2) : s_hat;   // dc.hpp:490-498
        stats = rslf_stats();
        epis_.assign(epis, epis + dim_v);
        type_ = type;
        row_stride_bytes_ = row_stride_bytes;
        epi_scale_arg_ = epi_scale_factor;
        scale_used_ = 255.f;
    }

    Context* ctx_;
    MultiContext* multi_;
    std::vector<const void*> epis_;   // multi path: the caller's buffers, read by run()
    InputType type_;
    size_t row_stride_bytes_;
    float epi_scale_arg_;
    rslf_volume* vol_;
    int dim_v_, dim_s_, dim_u_;
    int m_dim_d;
    float m_dmin, m_dmax;
    int m_s_hat;
    float scale_used_;
    bool subgrid_ = false;
    detail::Dilation dilation_;          // set_u_dilation
    Depth1DParameters m_parameters;      // (a copy: set_u_dilation scales its slope factor, the caller's object stays)
};

// rslf::Depth2DComputer<DataType> (dc.hpp:166-225, :651-805): disparities for every view, centre outwards,
// with propagation along EPI lines.  Results are dense [S][V][U] host vectors after run().
template <int CHANNELS>
class Depth2DComputer {
public:
    Depth2DComputer(Context& ctx, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                    float dmin, float dmax, int dim_d, float epi_scale_factor = -1,
                    const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : Depth2DComputer(ctx, epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d,
                          epi_scale_factor, parameters)
    {
    }
    Depth2DComputer(Context& ctx, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                    float dmin, float dmax, int dim_d, float epi_scale_factor = -1,
                    const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(&ctx), multi_(nullptr), vol_(nullptr), type_(type), stride_(row_stride_bytes), scale_(epi_scale_factor), dim_v_(dim_v),
          dim_s_(dim_s), dim_u_(dim_u), m_dim_d(dim_d), m_dmin(dmin), m_dmax(dmax), m_parameters(parameters)
    {
        stats = rslf_stats();
        check(rslf_volume_create(ctx_->get(), dim_v, dim_s, dim_u, CHANNELS, &vol_), "rslf_volume_create");
        detail::upload_epis(vol_, type, epis, row_stride_bytes, epi_scale_factor);
    }
    // The same on a MultiContext: the sweep is cut into one block of scanlines per device, the neighbours' boundary rows
    // exchanged by peer copy on every visit (rslf_multi_depth2d_run_*).  The EPIs are read by run(): they must outlive it.
    Depth2DComputer(MultiContext& multi, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                    float dmin, float dmax, int dim_d, float epi_scale_factor = -1,
                    const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : Depth2DComputer(multi, epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, dmin, dmax, dim_d,
                          epi_scale_factor, parameters)
    {
    }
    Depth2DComputer(MultiContext& multi, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u,
                    size_t row_stride_bytes, float dmin, float dmax, int dim_d, float epi_scale_factor = -1,
                    const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : ctx_(nullptr), multi_(&multi), vol_(nullptr), epis_(epis, epis + dim_v), type_(type), stride_(row_stride_bytes),
          scale_(epi_scale_factor), dim_v_(dim_v), dim_s_(dim_s), dim_u_(dim_u), m_dim_d(dim_d), m_dmin(dmin), m_dmax(dmax),
          m_parameters(parameters)
    {
        stats = rslf_stats();
    }
#ifdef RSLFX_HAVE_OPENCV
    // The reference's signature: Vec<Mat> in (dc.hpp:183-190), CV_8U, CV_16U or CV_32F.
    Depth2DComputer(Context& ctx, const std::vector<cv::Mat>& epis, float dmin, float dmax, int dim_d, float epi_scale_factor = -1,
                    const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : Depth2DComputer(ctx, detail::MatInput(epis, CHANNELS, "Depth2DComputer"), dmin, dmax, dim_d, epi_scale_factor, parameters)
    {
    }
    Depth2DComputer(MultiContext& multi, const std::vector<cv::Mat>& epis, float dmin, float dmax, int dim_d,
                    float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default())
        : Depth2DComputer(multi, detail::MatInput(epis, CHANNELS, "Depth2DComputer"), dmin, dmax, dim_d, epi_scale_factor, parameters)
    {
    }
#endif
    ~Depth2DComputer()
    {
        rslf_volume_destroy(vol_);
        if (dilation_.source != vol_)
            rslf_volume_destroy(dilation_.source);
    }
    Depth2DComputer(const Depth2DComputer&) = delete;
    Depth2DComputer& operator=(const Depth2DComputer&) = delete;

    void run()   // dc.hpp:748-805
    {
        const size_t n = (size_t)dim_s_ * dim_v_ * dim_u_;
        m_edge_confidence_s_v_u.assign(n, 0.f);
        m_edge_confidence_mask_s_v_u.assign(n, 0);
        m_disp_confidence_s_v_u.assign(n, 0.f);
        m_best_depth_s_v_u.assign(n, 0.f);
        m_rbar_s_v_u.assign(n * CHANNELS, 0.f);
        const rslf_params p = m_parameters.to_c();
        const int line_mode = m_parameters.par_line_confidence_mode;
        detail::require(!multi_ || line_mode == RSLF_LINE_CONF_OFF, "Depth2DComputer: line confidence runs on one device");
        // K7 samples C_e along u + (s_hat - s) * d with no slope factor (core.hpp:1058): in a dilated frame it would walk the wrong line
        detail::require(dilation_.factor == 1 || line_mode == RSLF_LINE_CONF_OFF,
                        "Depth2DComputer: par_line_confidence_mode together with set_u_dilation is not built (the line confidence takes no slope factor)");
        detail::require(peaks_ || propagation_ratio_ == 0.f, "Depth2DComputer: the propagation ratio reads the peak planes: call set_peaks(true)");
        withheld_ = 0;
        if (multi_) {
            if (type_ == InputType::U8)
                check(rslf_multi_depth2d_run_u8(multi_->get(), (const uint8_t* const*)epis_.data(), stride_, dim_v_, dim_s_, dim_u_, CHANNELS,
                                                m_dmin, m_dmax, m_dim_d, &p, m_edge_confidence_s_v_u.data(),
                                                m_edge_confidence_mask_s_v_u.data(), m_disp_confidence_s_v_u.data(),
                                                m_best_depth_s_v_u.data(), m_rbar_s_v_u.data(), nullptr, &stats),
                      "rslf_multi_depth2d_run_u8");
            else if (type_ == InputType::U16)
                check(rslf_multi_depth2d_run_u16(multi_->get(), (const uint16_t* const*)epis_.data(), stride_, dim_v_, dim_s_, dim_u_,
                                                 CHANNELS, scale_, m_dmin, m_dmax, m_dim_d, &p, m_edge_confidence_s_v_u.data(),
                                                 m_edge_confidence_mask_s_v_u.data(), m_disp_confidence_s_v_u.data(),
                                                 m_best_depth_s_v_u.data(), m_rbar_s_v_u.data(), nullptr, &stats, nullptr),
                      "rslf_multi_depth2d_run_u16");
            else
                check(rslf_multi_depth2d_run_f32(multi_->get(), (const float* const*)epis_.data(), stride_, dim_v_, dim_s_, dim_u_, CHANNELS,
                                                 scale_, m_dmin, m_dmax, m_dim_d, &p, m_edge_confidence_s_v_u.data(),
                                                 m_edge_confidence_mask_s_v_u.data(), m_disp_confidence_s_v_u.data(),
                                                 m_best_depth_s_v_u.data(), m_rbar_s_v_u.data(), nullptr, &stats, nullptr),
                      "rslf_multi_depth2d_run_f32");
            return;
        }
        if (line_mode != RSLF_LINE_CONF_OFF)   // dc.hpp:721-738, :791-792
            m_line_confidence_s_v_u.assign(n, 0.f);
        rslf_peaks planes = {};
        if (peaks_) {   // every visit in the peaks mode (rslf_sweep_peaks)
            peaks_s_v_u_.idx.assign(n, -1), peaks_s_v_u_.runner_idx.assign(n, -1);
            peaks_s_v_u_.score.assign(n, 0.f), peaks_s_v_u_.runner_score.assign(n, 0.f);
            planes.idx = peaks_s_v_u_.idx.data(), planes.score = peaks_s_v_u_.score.data();
            planes.runner_idx = peaks_s_v_u_.runner_idx.data(), planes.runner_score = peaks_s_v_u_.runner_score.data();
        }
        // the family's widest entry: a mode that is off goes in neutral, and the call is the narrower entry's (rslf_hip.h)
        check(rslf_depth2d_run_host_pr(ctx_->get(), vol_, m_dmin, m_dmax, m_dim_d, &p, m_edge_confidence_s_v_u.data(),
                                       m_edge_confidence_mask_s_v_u.data(), m_disp_confidence_s_v_u.data(), m_best_depth_s_v_u.data(),
                                       m_rbar_s_v_u.data(), &stats, line_mode,
                                       line_mode != RSLF_LINE_CONF_OFF ? m_line_confidence_s_v_u.data() : nullptr, subgrid_ ? 1 : 0,
                                       peaks_ ? &planes : nullptr, propagation_ratio_),
              "rslf_depth2d_run_host_pr");
        if (propagation_ratio_ != 0.f)   // gated by the peak ratio (rslf_sweep_propagation_ratio): what it withheld
            check(rslf_sweep_withheld(ctx_->get(), &withheld_), "rslf_sweep_withheld");
    }
    // Not in the reference: with the mode on, every visit of run() moves the disparities its scan assigns off the hypothesis
    // grid (rslf_sweep_subgrid, rslf_hip.h) before the selective median and the propagation read them; m_best_depth_s_v_u
    // and the pictures of every getter then hold refined values.  Default off.  One context: an object built on a
    // MultiContext throws with the mode on, as Depth1DComputer_pile::set_subgrid does.
    void set_subgrid(bool on)
    {
        if (on && multi_)
            throw std::invalid_argument("set_subgrid: this object was built on a MultiContext: the sub-grid mode is built for one context");
        subgrid_ = on;
    }
    bool get_subgrid() const { return subgrid_; }
    // Not in the reference's code, to be called before run(): as Depth1DComputer_pile::set_u_dilation.  The sweep, its
    // propagation, get_consistency, get_warped_view, get_view_prediction, get_novel_view and the pictures all answer in the
    // dilated frame, u_dilated() columns wide, with the slope factor par_slope_factor * factor.  Refused together with a line
    // confidence mode (by run()).  One context: throws on a MultiContext.
    void set_u_dilation(int factor, int kind = RSLF_DILATE_CUBIC)
    {
        detail::set_u_dilation(dilation_, multi_ ? nullptr : ctx_, vol_, dim_u_, m_parameters.par_slope_factor, factor, kind);
        m_edge_confidence_s_v_u.clear(), m_edge_confidence_mask_s_v_u.clear(), m_disp_confidence_s_v_u.clear(), m_best_depth_s_v_u.clear();
        m_rbar_s_v_u.clear(), m_line_confidence_s_v_u.clear();
        peaks_s_v_u_ = Peaks();
    }
    int get_u_dilation() const { return dilation_.factor; }
    int u_dilated() const { return dim_u_; }
    // get_depths_s_v_u() and get_valid_depths_mask_s_v_u() on the source grid, [S][V][U]: their columns u * factor.
    std::vector<float> get_depths_undilated() const { return detail::undilated(m_best_depth_s_v_u, dim_u_, dilation_.factor); }
    std::vector<uint8_t> get_valid_depths_mask_undilated() const
    {
        return detail::undilated(get_valid_depths_mask_s_v_u(), dim_u_, dilation_.factor);
    }
    // Not in the reference: with the mode on, run() also fills, for every view, the winner and the runner-up peak of the score
    // row of every pixel a visit scanned and accepted, and a painted pixel takes its source's (rslf_sweep_peaks, rslf_hip.h);
    // a pixel no visit scanned or painted holds -1 / 0.  No other plane changes.  Default off.  One context: an object built
    // on a MultiContext throws, as Depth1DComputer_pile::get_peaks does.
    struct Peaks {
        std::vector<int32_t> idx, runner_idx;      // [S][V][U]
        std::vector<float> score, runner_score;
    };
    void set_peaks(bool on)
    {
        if (on && multi_)
            throw std::invalid_argument("set_peaks: this object was built on a MultiContext: the sweep's peaks are built for one context");
        peaks_ = on;
    }
    const Peaks& get_peaks() const
    {
        if (multi_)
            throw std::invalid_argument("get_peaks: this object was built on a MultiContext: the sweep's peaks are built for one context");
        if (!peaks_)
            throw std::invalid_argument("get_peaks: the mode is off: set_peaks(true) before run()");
        detail::require(!peaks_s_v_u_.idx.empty(), "the getters show the results of run(): call it first");
        return peaks_s_v_u_;
    }
    // Not in the reference: the sweep gate (rslf_sweep_propagation_ratio, rslf_hip.h).  ratio in (0, 1], 0 switches it off:
    // a pixel whose runner-up scores more than ratio * its winner is withheld from propagation -- no claim, its raw
    // disparity, still in the running mask.  Needs set_peaks(true) by the time run() is called.  After run():
    // get_withheld_sources, the sources the sweep withheld (0 without the ratio).  On a MultiContext throws, as set_peaks.
    void set_propagation_ratio(float ratio)
    {
        if (ratio != 0.f && multi_)
            throw std::invalid_argument("set_propagation_ratio: this object was built on a MultiContext: the sweep gate is built for one context");
        detail::require(ratio >= 0.f && ratio <= 1.f, "propagation ratio: 0 (off) or a ratio in (0, 1]");
        propagation_ratio_ = ratio;
    }
    float get_propagation_ratio() const { return propagation_ratio_; }
    unsigned long long get_withheld_sources() const
    {
        if (multi_)
            throw std::invalid_argument("get_withheld_sources: this object was built on a MultiContext: the sweep gate is built for one context");
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        return withheld_;
    }
    const std::vector<float>& get_depths_s_v_u() const { return m_best_depth_s_v_u; }
    // dc.hpp:893-915, default build: C_e > edge threshold -- or, with RSLF_LINE_CONF_GATE and without
    // par_use_disp_confidence_score, C_l > line threshold (dc.hpp:904)
    std::vector<uint8_t> get_valid_depths_mask_s_v_u() const
    {
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        const bool by_line = !m_parameters.par_use_disp_confidence_score && m_parameters.par_line_confidence_mode == RSLF_LINE_CONF_GATE;
        const std::vector<float>& score = by_line ? m_line_confidence_s_v_u : m_edge_confidence_s_v_u;
        const float thr = by_line ? m_parameters.par_line_score_threshold : m_parameters.par_edge_score_threshold;
        std::vector<uint8_t> mask(score.size());
        for (size_t i = 0; i < mask.size(); i++)
            mask[i] = score[i] > thr ? 255 : 0;
        return mask;
    }
    // Not in the reference: after run(), do the views agree with one another (rslf_view_consistency_host, rslf_hip.h)?  The
    // disparity planes with the sweep's own slope factor; tol < 0: one step of the hypothesis grid, (dmax - dmin) / (dim_d - 1);
    // mask (nullable, [S][V][U]): get_valid_depths_mask_s_v_u().  An object built on a MultiContext takes the Context to run on.
    Consistency get_consistency(Context& on, float tol = -1.f, int radius = 0, int min_agree = 0, const uint8_t* mask = nullptr) const
    {
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        std::vector<uint8_t> own_mask;
        if (!mask) {
            own_mask = get_valid_depths_mask_s_v_u();
            mask = own_mask.data();
        }
        Consistency out;
        const rslf_view_counts counts = detail::consistency_planes(out, m_best_depth_s_v_u.size());
        check(rslf_view_consistency_host(on.get(), m_best_depth_s_v_u.data(), mask, dim_s_, dim_v_, dim_u_, m_parameters.par_slope_factor,
                                         tol < 0.f ? detail::grid_step(m_dmin, m_dmax, m_dim_d) : tol, radius, min_agree, &counts,
                                         out.fused.data(), out.valid.data()),
              "rslf_view_consistency_host");
        return out;
    }
    Consistency get_consistency(float tol = -1.f, int radius = 0, int min_agree = 0, const uint8_t* mask = nullptr) const
    {
        return get_consistency(detail::own(ctx_), tol, radius, min_agree, mask);
    }

    // Not in the reference: after run(), the view at position `target` (a float: it need not be a view, nor inside the range)
    // as the disparity planes of the views predict it (rslf_view_warp_host, rslf_hip.h): every source pixel is sent to its
    // column in the target and the nearest wins (nearer = +1: the largest disparity, so one wrong large value wins its pixel;
    // -1: the smallest).  exclude: a view that takes no part (-1: nobody); radius > 0: only views within it; mask (nullable,
    // [S][V][U]): get_valid_depths_mask_s_v_u().  colour reads the object's volume, which an object built on a MultiContext
    // does not hold; such an object takes the Context to run on.  -> planes [1][V][U].
    Warp get_warped_view(Context& on, float target, int exclude = -1, int radius = 0, int nearer = 1, const uint8_t* mask = nullptr,
                         bool colour = true) const
    {
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        detail::require(!colour || vol_ != nullptr, "get_warped_view: colour reads the volume, which an object built on a MultiContext does not hold");
        std::vector<uint8_t> own_mask;
        if (!mask) {
            own_mask = get_valid_depths_mask_s_v_u();
            mask = own_mask.data();
        }
        Warp out;
        const rslf_view_warp_out planes = detail::warp_planes(out, (size_t)dim_v_ * dim_u_, CHANNELS, colour);
        check(rslf_view_warp_host(on.get(), m_best_depth_s_v_u.data(), mask, dim_s_, dim_v_, dim_u_, m_parameters.par_slope_factor,
                                  colour ? vol_ : nullptr, &target, &exclude, 1, radius, nearer, &planes),
              "rslf_view_warp_host");
        return out;
    }
    Warp get_warped_view(float target, int exclude = -1, int radius = 0, int nearer = 1, const uint8_t* mask = nullptr, bool colour = true) const
    {
        return get_warped_view(detail::own(ctx_), target, exclude, radius, nearer, mask, colour);
    }
    // ... and the leave-one-out yardstick: the views `views` (empty: all of them), each predicted from the others and compared
    // with the view that was taken.  It judges a mask or a parameter choice without ground-truth depth.
    ViewPrediction get_view_prediction(Context& on, std::vector<int> views = std::vector<int>(), int radius = 0, int nearer = 1,
                                       const uint8_t* mask = nullptr) const
    {
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        detail::require(vol_ != nullptr, "get_view_prediction reads the volume, which an object built on a MultiContext does not hold");
        std::vector<uint8_t> own_mask;
        if (!mask) {
            own_mask = get_valid_depths_mask_s_v_u();
            mask = own_mask.data();
        }
        const std::vector<float> targets = detail::prediction_targets(views, dim_s_);
        ViewPrediction out;
        const rslf_view_warp_out planes = detail::prediction_planes(out, (int)views.size(), dim_v_, dim_u_);
        check(rslf_view_warp_host(on.get(), m_best_depth_s_v_u.data(), mask, dim_s_, dim_v_, dim_u_, m_parameters.par_slope_factor, vol_,
                                  targets.data(), views.data(), (int)views.size(), radius, nearer, &planes),
              "rslf_view_warp_host");
        detail::prediction_finish(out, (int)views.size(), dim_v_, dim_u_);
        return out;
    }
    ViewPrediction get_view_prediction(std::vector<int> views = std::vector<int>(), int radius = 0, int nearer = 1,
                                       const uint8_t* mask = nullptr) const
    {
        return get_view_prediction(detail::own(ctx_), views, radius, nearer, mask);
    }
    // Not in the reference: after run(), the view at position `target` as a finished image (rslf_novel_view_host, rslf_hip.h):
    // the warp's z-buffer, its holes filled from the farther bound, and every pixel's colour gathered backwards from the views
    // that agree with its disparity, blended at sub-pixel columns.  mask as get_warped_view's.  An object built on a
    // MultiContext takes the Context to run on and holds no volume: it gives depth, fill and n_src only (colour = false).
    NovelView get_novel_view(Context& on, float target, int exclude = -1, const NovelViewOptions& options = NovelViewOptions(),
                             const uint8_t* mask = nullptr, bool colour = true) const
    {
        detail::require(!m_best_depth_s_v_u.empty(), "the getters show the results of run(): call it first");
        detail::require(!colour || vol_ != nullptr, "get_novel_view: colour reads the volume, which an object built on a MultiContext does not hold");
        std::vector<uint8_t> own_mask;
        if (!mask) {
            own_mask = get_valid_depths_mask_s_v_u();
            mask = own_mask.data();
        }
        NovelView out;
        const rslf_novel_view_out planes = detail::novel_planes(out, (size_t)dim_v_ * dim_u_, CHANNELS, colour);
        const rslf_novel_view_params params = detail::novel_params(options, options.tol < 0.f ? detail::grid_step(m_dmin, m_dmax, m_dim_d) : 0.f);
        check(rslf_novel_view_host(on.get(), m_best_depth_s_v_u.data(), mask, dim_s_, dim_v_, dim_u_, m_parameters.par_slope_factor,
                                   colour ? vol_ : nullptr, &target, &exclude, 1, &params, &planes),
              "rslf_novel_view_host");
        return out;
    }
    NovelView get_novel_view(float target, int exclude = -1, const NovelViewOptions& options = NovelViewOptions(), const uint8_t* mask = nullptr,
                             bool colour = true) const
    {
        return get_novel_view(detail::own(ctx_), target, exclude, options, mask, colour);
    }

    // dc.hpp:808-856: the S x U slice of the disparities at scanline a_v (< 0: floor(V / 2.0)) over its own min / max,
    // colour-mapped, black outside the mask; no line drawing -> [S][U][3].  The slice is read through its row stride.
    std::vector<uint8_t> get_coloured_epi(Context& on, int a_v, const uint8_t* lut_bgr) const
    {
        if (a_v < 0)
            a_v = (int)std::floor(dim_v_ / 2.0);
        detail::require(a_v < dim_v_, "get_coloured_epi: the scanline is not below dim_v");
        return slices(on, (size_t)a_v * dim_u_, 1, 0, dim_s_, (size_t)dim_v_ * dim_u_, lut_bgr);
    }
    std::vector<uint8_t> get_coloured_epi(int a_v, const uint8_t* lut_bgr) const { return get_coloured_epi(detail::own(ctx_), a_v, lut_bgr); }
    // dc.hpp:858-891: view a_s (< 0: floor(S / 2.0)) over its min / max (every pixel), colour-mapped, black outside the
    // mask -> [V][U][3]
    std::vector<uint8_t> get_disparity_map(Context& on, int a_s, const uint8_t* lut_bgr) const
    {
        if (a_s < 0)
            a_s = (int)std::floor(dim_s_ / 2.0);
        detail::require(a_s < dim_s_, "get_disparity_map: the view is not below dim_s");
        return slices(on, (size_t)a_s * dim_v_ * dim_u_, 1, 0, dim_v_, (size_t)dim_u_, lut_bgr);
    }
    std::vector<uint8_t> get_disparity_map(int a_s, const uint8_t* lut_bgr) const { return get_disparity_map(detail::own(ctx_), a_s, lut_bgr); }
    // get_disparity_map(a_s) for every view (the loop of the reference's demo, tests/test_depth_computation_2d.cpp:77)
    // -> [S][V][U][3], and get_coloured_epi(a_v) for every scanline -> [V][S][U][3]: one upload, one batch of fits, one
    // render launch, each plane over its own min / max.
    std::vector<uint8_t> get_disparity_maps(Context& on, const uint8_t* lut_bgr) const
    {
        return slices(on, 0, dim_s_, (size_t)dim_v_ * dim_u_, dim_v_, (size_t)dim_u_, lut_bgr);
    }
    std::vector<uint8_t> get_disparity_maps(const uint8_t* lut_bgr) const { return get_disparity_maps(detail::own(ctx_), lut_bgr); }
    std::vector<uint8_t> get_coloured_epis(Context& on, const uint8_t* lut_bgr) const
    {
        return slices(on, 0, dim_v_, (size_t)dim_u_, dim_s_, (size_t)dim_v_ * dim_u_, lut_bgr);
    }
    std::vector<uint8_t> get_coloured_epis(const uint8_t* lut_bgr) const { return get_coloured_epis(detail::own(ctx_), lut_bgr); }

    std::vector<float> m_edge_confidence_s_v_u;
    std::vector<uint8_t> m_edge_confidence_mask_s_v_u;
    std::vector<float> m_disp_confidence_s_v_u;
    std::vector<float> m_line_confidence_s_v_u;   // filled with par_line_confidence_mode >= 1 (dc.hpp:737), else empty
    std::vector<float> m_rbar_s_v_u;
    std::vector<float> m_best_depth_s_v_u;
    rslf_stats stats;

private:
#ifdef RSLFX_HAVE_OPENCV
    template <typename Ctx>
    Depth2DComputer(Ctx& ctx, const detail::MatInput& in, float dmin, float dmax, int dim_d, float epi_scale_factor,
                    const Depth1DParameters& parameters)
        : Depth2DComputer(ctx, in.ptrs.data(), in.type, in.V, in.S, in.U, in.stride, dmin, dmax, dim_d, epi_scale_factor, parameters)
    {
    }
#endif
    // n planes of rows x dim_u out of the [S][V][U] results, under the mask the getters paint with: the edge mask in the
    // default build (dc.hpp:840-842, :885-887); with par_use_disp_confidence_score, C_d > (float)par_disp_score_threshold
    // (:832-834, :875-878); else with RSLF_LINE_CONF_GATE, C_l > (float)par_line_score_threshold (:842, :883)
    std::vector<uint8_t> slices(Context& on, size_t offset, int n, size_t plane_stride, int rows, size_t row_stride, const uint8_t* lut_bgr) const
    {
        std::vector<uint8_t> by_score;
        if (m_parameters.par_use_disp_confidence_score) {
            by_score.resize(m_disp_confidence_s_v_u.size());
            for (size_t i = 0; i < by_score.size(); i++)
                by_score[i] = m_disp_confidence_s_v_u[i] > m_parameters.par_disp_score_threshold ? 255 : 0;
        }
        const bool by_line = !m_parameters.par_use_disp_confidence_score && m_parameters.par_line_confidence_mode == RSLF_LINE_CONF_GATE;
        if (by_line) {
            detail::require(m_line_confidence_s_v_u.size() == m_best_depth_s_v_u.size(), "the line confidence is filled by run()");
            by_score.resize(m_line_confidence_s_v_u.size());
            for (size_t i = 0; i < by_score.size(); i++)
                by_score[i] = m_line_confidence_s_v_u[i] > m_parameters.par_line_score_threshold ? 255 : 0;
        }
        const std::vector<uint8_t>& mask = (m_parameters.par_use_disp_confidence_score || by_line) ? by_score : m_edge_confidence_mask_s_v_u;
        return detail::render_planes(on.get(), m_best_depth_s_v_u, offset, mask.data(), n, plane_stride, rows, dim_u_, row_stride,
                                     RSLF_FIT_MINMAX, -1, RSLF_RENDER_SHIFT, lut_bgr);
    }

    Context* ctx_;
    MultiContext* multi_;
    rslf_volume* vol_;
    std::vector<const void*> epis_;
    InputType type_;
    size_t stride_;
    float scale_;
    int dim_v_, dim_s_, dim_u_, m_dim_d;
    float m_dmin, m_dmax;
    Depth1DParameters m_parameters;      // (a copy: set_u_dilation scales its slope factor, the caller's object stays)
    detail::Dilation dilation_;          // set_u_dilation
    bool subgrid_ = false;   // set_subgrid
    bool peaks_ = false;     // set_peaks
    Peaks peaks_s_v_u_;      // filled by run() with the mode on
    float propagation_ratio_ = 0.f;      // set_propagation_ratio
    unsigned long long withheld_ = 0;    // what run() withheld (0 without the ratio)
};

// rslf::FineToCoarse<DataType> (include/rslf_fine_to_coarse.hpp:26-81): constructor arguments as in the
// reference; run() builds the pyramid, sweeps every level and fuses; get_results() hands out the fused maps.
template <int CHANNELS>
class FineToCoarse {
public:
    FineToCoarse(Context& ctx, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                 float d_min, float d_max, int dim_d, float epi_scale_factor = -1,
                 const Depth1DParameters& parameters = Depth1DParameters::get_default(), int max_pyr_depth = -1,
                 bool accept_all_last_scale = true)
        : FineToCoarse(&ctx, nullptr, epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, d_min, d_max,
                       dim_d, epi_scale_factor, parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
    // The same with the element type named: InputType::U16 keeps ushort arithmetic through the pyramid, as the reference's
    // CV_16U Mats do (rslf_fine_to_coarse_run_host_u16).
    FineToCoarse(Context& ctx, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                 float d_min, float d_max, int dim_d, float epi_scale_factor = -1,
                 const Depth1DParameters& parameters = Depth1DParameters::get_default(), int max_pyr_depth = -1,
                 bool accept_all_last_scale = true)
        : FineToCoarse(&ctx, nullptr, epis, type, dim_v, dim_s, dim_u, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor,
                       parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
    // The same over a MultiContext's devices: every level's sweep sharded by scanline (rslf_multi_fine_to_coarse_run_host).
    FineToCoarse(MultiContext& multi, const void* const* epis, bool is_u8, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                 float d_min, float d_max, int dim_d, float epi_scale_factor = -1,
                 const Depth1DParameters& parameters = Depth1DParameters::get_default(), int max_pyr_depth = -1,
                 bool accept_all_last_scale = true)
        : FineToCoarse(nullptr, &multi, epis, is_u8 ? InputType::U8 : InputType::F32, dim_v, dim_s, dim_u, row_stride_bytes, d_min,
                       d_max, dim_d, epi_scale_factor, parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
    FineToCoarse(MultiContext& multi, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u, size_t row_stride_bytes,
                 float d_min, float d_max, int dim_d, float epi_scale_factor = -1,
                 const Depth1DParameters& parameters = Depth1DParameters::get_default(), int max_pyr_depth = -1,
                 bool accept_all_last_scale = true)
        : FineToCoarse(nullptr, &multi, epis, type, dim_v, dim_s, dim_u, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor,
                       parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
#ifdef RSLFX_HAVE_OPENCV
    // The reference's signature: Vec<Mat> in (rslf_fine_to_coarse.hpp:103-110), CV_8U, CV_16U or CV_32F.
    FineToCoarse(Context& ctx, const std::vector<cv::Mat>& epis, float d_min, float d_max, int dim_d, float epi_scale_factor = -1,
                 const Depth1DParameters& parameters = Depth1DParameters::get_default(), int max_pyr_depth = -1,
                 bool accept_all_last_scale = true)
        : FineToCoarse(&ctx, nullptr, detail::MatInput(epis, CHANNELS, "FineToCoarse"), d_min, d_max, dim_d, epi_scale_factor,
                       parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
    FineToCoarse(MultiContext& multi, const std::vector<cv::Mat>& epis, float d_min, float d_max, int dim_d,
                 float epi_scale_factor = -1, const Depth1DParameters& parameters = Depth1DParameters::get_default(),
                 int max_pyr_depth = -1, bool accept_all_last_scale = true)
        : FineToCoarse(nullptr, &multi, detail::MatInput(epis, CHANNELS, "FineToCoarse"), d_min, d_max, dim_d, epi_scale_factor,
                       parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
#endif
    // The -D_USE_LINE_CONFIDENCE_SCORE build of the pyramid, to be called before run(): every level's sweep runs in `mode`
    // (RSLF_LINE_CONF_*) with a C_l plane of its own, and with RSLF_LINE_CONF_GATE (without par_use_disp_confidence_score)
    // each level's validity is C_l > par_line_score_threshold (dc.hpp:903-904).  run() then also keeps every level's
    // disparities, validity and line confidence for the per-level getters.  One device only.
    void set_line_confidence_mode(int mode)
    {
        detail::require(!multi_, "FineToCoarse: line confidence runs on one device");
        detail::require(mode >= RSLF_LINE_CONF_OFF && mode <= RSLF_LINE_CONF_GATE, "line confidence mode: RSLF_LINE_CONF_OFF, _AS_BUILT or _GATE");
        line_mode_ = mode;
    }
    // The dilation along u (Depth2DComputer::set_u_dilation) is not built for the pyramid's LEVELS -- they would need a decision
    // about uchar arithmetic in dilated levels and about the width the pyramid starts from: any factor but 1 throws.  The
    // pyramid's form is set_level_dilation below, which dilates each level's sweep alone.
    void set_u_dilation(int factor, int kind = RSLF_DILATE_CUBIC)
    {
        (void)kind;
        if (factor != 1)
            throw std::invalid_argument("set_u_dilation: the dilation along u is not built for FineToCoarse (one level: Depth1DComputer_pile, Depth2DComputer)");
    }
    // Not in the reference's code (its report's fourth lead), to be called before run(): the level dilation
    // (rslf_fine_to_coarse_run_host_dl, rslf_f2c_run_host_dl; rslf_hip.h "the level dilation").  Every level's SWEEP runs on the
    // level's volume dilated along u by `factor` (1..8, kernel `kind`) with the slope factor times the factor, and its planes
    // come back to the level's own grid before anything reads them: every result of this object keeps its shape, and the
    // level chain is untouched.  1 switches it off.  Any other factor throws on a MultiContext (one device); a
    // line-confidence mode together with it is refused by run().
    void set_level_dilation(int factor, int kind = RSLF_DILATE_CUBIC)
    {
        if (factor < 1 || factor > 8)
            throw std::invalid_argument("set_level_dilation: a factor in 1..8");
        if (kind != RSLF_DILATE_LINEAR && kind != RSLF_DILATE_CUBIC && kind != RSLF_DILATE_LANCZOS3)
            throw std::invalid_argument("set_level_dilation: RSLF_DILATE_LINEAR, RSLF_DILATE_CUBIC or RSLF_DILATE_LANCZOS3");
        if (factor != 1 && multi_)
            throw std::invalid_argument("set_level_dilation: this object was built on a MultiContext: the level dilation is built for one context");
        level_dilation_ = factor;
        level_dilation_kind_ = kind;
    }
    int get_level_dilation() const { return level_dilation_; }
    int get_level_dilation_kind() const { return level_dilation_kind_; }
    // Not in the reference's code (its report's second lead), to be called before run(): the derivative channels
    // (rslf_fine_to_coarse_run_host_dv, rslf_f2c_run_host_dv; rslf_hip.h "derivative channels").  A one-channel field goes down
    // the pyramid as (x, min(|dx/du| * weight / 2, hi), min(|dx/dv| * weight / 2, hi)), made once on the device from the
    // finest level, and every level runs as it does for a three-channel field, bit for bit; a kept run is a three-channel
    // run (its renderers' shadow cut takes the norm of three channels, get_coloured_epi_pyr's volumes hold the features;
    // without a kept run the shadow cut of get_coloured_depth_maps reads the EPIs as they were given).  0 switches it off.
    // Any other weight throws on an RGB field (one channel and two features are three) and on a MultiContext (one device).
    void set_derivative_channels(float weight)
    {
        if (weight != 0.f && CHANNELS != 1)
            throw std::invalid_argument("set_derivative_channels: the derivative channels are built for a one-channel field (FineToCoarse<1>)");
        if (weight != 0.f && multi_)
            throw std::invalid_argument("set_derivative_channels: this object was built on a MultiContext: the derivative channels are built for one context");
        if (!(weight >= 0.f && weight <= 3.402823466e+38f))
            throw std::invalid_argument("set_derivative_channels: 0 (off) or a finite weight > 0");
        derivative_weight_ = weight;
    }
    float get_derivative_channels() const { return derivative_weight_; }
    // Not in the reference's code (the remedy its report names for global changes of illumination between frames), to be
    // called before run(): the per-view equalisation (rslf_fine_to_coarse_run_host_eq, rslf_f2c_run_host_eq; rslf_hip.h
    // "per-view equalisation").  The finest level's upload is equalised on the device, y = a x + b with one (a, b) per view
    // and channel, before the derivative channels, and the pyramid runs on it bit for bit as on the equalised field.  mode:
    // RSLF_EQUALIZE_GAIN or RSLF_EQUALIZE_AFFINE, 0 switches it off; ref_view: the view whose statistics are the target,
    // -1 the views' mean, -2 (the default) the centre view dim_s / 2, where the sweep starts; joint: one pair for the three
    // channels of an RGB field, -1 (the default) on for FineToCoarse<3>; max_gain: the clamp of the gain.  Any mode but 0
    // throws on a MultiContext (one device: a view's statistic spans all scanlines).
    void set_equalize_views(int mode, int ref_view = -2, int joint = -1, float max_gain = 4.f)
    {
        if (mode != 0 && mode != RSLF_EQUALIZE_GAIN && mode != RSLF_EQUALIZE_AFFINE)
            throw std::invalid_argument("set_equalize_views: 0 (off), RSLF_EQUALIZE_GAIN or RSLF_EQUALIZE_AFFINE");
        if (mode != 0 && multi_)
            throw std::invalid_argument("set_equalize_views: this object was built on a MultiContext: the per-view equalisation is built for one context");
        if (ref_view == -2)
            ref_view = dim_s_ / 2;
        if (joint < 0)
            joint = CHANNELS == 3 ? 1 : 0;
        if (mode != 0) {
            if (ref_view < -1 || ref_view >= dim_s_)
                throw std::invalid_argument("set_equalize_views: ref_view is -1 (the views' mean) or a view in [0, dim_s)");
            if (joint && CHANNELS != 3)
                throw std::invalid_argument("set_equalize_views: joint is built for a three-channel field (FineToCoarse<3>)");
            if (!(max_gain >= 1.f && max_gain <= 3.402823466e+38f))
                throw std::invalid_argument("set_equalize_views: max_gain is a finite gain >= 1");
        }
        equalize_mode_ = mode, equalize_ref_view_ = ref_view, equalize_joint_ = joint ? 1 : 0, equalize_max_gain_ = max_gain;
    }
    int get_equalize_views() const { return equalize_mode_; }
    // The coefficients a kept run's equalisation applied, [dim_s][CHANNELS][2] (a, b); empty for a run made without it
    // and without a kept run (keep_on_device): the host-planes entries hand no coefficients out.
    std::vector<float> get_view_gains() const
    {
        std::vector<float> a_b;
        int mode = 0;
        if (run_)
            check(rslf_f2c_run_equalize(run_, &mode, nullptr, nullptr), "rslf_f2c_run_equalize");
        if (mode != 0) {
            a_b.resize((size_t)dim_s_ * CHANNELS * 2);
            check(rslf_f2c_run_equalize(run_, nullptr, nullptr, a_b.data()), "rslf_f2c_run_equalize");
        }
        return a_b;
    }
    // To be called before run(): the run stays on the device (rslf_f2c_run_host) and this object owns it.  get_results()
    // copies the fused planes out, the coloured getters are rendered there from the kept planes -- nothing is uploaded a
    // second time --, get_coloured_depth_pyr works in every line mode, get_coloured_epi_pyr exists, and the per-level
    // getters fill from the device when first asked.  keep_volumes: every level keeps the volume its sweep ran on, which
    // the shadow cut of get_coloured_depth_maps / get_coloured_epi_pyr reads (par_cut_shadows).  One device only.
    void keep_on_device(bool keep_volumes = true)
    {
        detail::require(!multi_, "FineToCoarse: a kept run lives on one device");
        keep_ = true;
        keep_volumes_ = keep_volumes;
    }
    // RSLF_F2C_VALID_COMPAT (what every other path computes) or RSLF_F2C_VALID_REFERENCE (the whole chain of
    // get_valid_depths_mask_s_v_u, validity by C_d under par_use_disp_confidence_score included); after keep_on_device.
    void set_validity_rule(int rule)
    {
        detail::require(keep_, "FineToCoarse: the validity rule belongs to a kept run: call keep_on_device first");
        detail::require(rule == RSLF_F2C_VALID_COMPAT || rule == RSLF_F2C_VALID_REFERENCE, "validity rule: RSLF_F2C_VALID_COMPAT or _REFERENCE");
        validity_rule_ = rule;
    }
    // Not in the reference, to be called before run(): every level's sweep runs in the sub-grid mode (rslf_sweep_subgrid), so
    // the coarser levels' ranges are tightened from off-grid disparities and every getter shows refined planes.  run() then
    // also keeps every level's planes, as after set_line_confidence_mode.  One device only: throws on a MultiContext.
    void set_subgrid(bool on)
    {
        if (on && multi_)
            throw std::invalid_argument("set_subgrid: this object was built on a MultiContext: the sub-grid mode is built for one context");
        subgrid_ = on;
    }
    bool get_subgrid() const { return subgrid_; }
    // Not in the reference, to be called before run() and after keep_on_device: every level's sweep also runs in the peaks
    // mode (rslf_sweep_peaks) and the kept run holds every level's peak planes and the fused peaks (rslf_f2c_run_host_pk).
    // One device only: throws on a MultiContext.
    struct Peaks {
        std::vector<int32_t> idx, runner_idx;      // [S][V_p][U_p]
        std::vector<float> score, runner_score;
    };
    void set_peaks(bool on)
    {
        if (multi_)
            throw std::invalid_argument("set_peaks: this object was built on a MultiContext: the pyramid's peaks are built for one context");
        detail::require(keep_, "FineToCoarse: the peak planes belong to a kept run: call keep_on_device first");
        peaks_ = on;
    }
    bool get_peaks_mode() const { return peaks_; }
    // ... and validity by uniqueness: ratio in (0, 1], 0 switches it off.  A level's valid pixels whose runner-up scores more
    // than ratio * the winner's score become invalid (the level accept_all_last_scale accepts whole apart), so the next
    // level's ranges and the fusion leave them to a coarser level.  Needs set_peaks(true) by the time run() is called.
    void set_uniqueness_ratio(float ratio)
    {
        if (multi_)
            throw std::invalid_argument("set_uniqueness_ratio: this object was built on a MultiContext: the pyramid's peaks are built for one context");
        detail::require(keep_, "FineToCoarse: the uniqueness ratio belongs to a kept run: call keep_on_device first");
        detail::require(ratio >= 0.f && ratio <= 1.f, "uniqueness ratio: 0 (off) or a ratio in (0, 1]");
        uniqueness_ = ratio;
    }
    float get_uniqueness_ratio() const { return uniqueness_; }
    // ... and the sweep gate of every level (rslf_f2c_run_host_pr): ratio in (0, 1], 0 switches it off.  Independent of the
    // uniqueness ratio; a kept run only, and it needs set_peaks(true) by the time run() is called.  After run():
    // get_withheld_sources(level), the sources that level's sweep withheld.
    void set_propagation_ratio(float ratio)
    {
        if (ratio != 0.f && multi_)
            throw std::invalid_argument("set_propagation_ratio: this object was built on a MultiContext: the sweep gate is built for one context");
        detail::require(keep_, "FineToCoarse: the propagation ratio belongs to a kept run: call keep_on_device first");
        detail::require(ratio >= 0.f && ratio <= 1.f, "propagation ratio: 0 (off) or a ratio in (0, 1]");
        propagation_ratio_ = ratio;
    }
    float get_propagation_ratio() const { return propagation_ratio_; }
    unsigned long long get_withheld_sources(int level) const
    {
        detail::require(run_ != nullptr, "get_withheld_sources: the counts are held by a kept run: keep_on_device, then run()");
        unsigned long long n = 0;
        check(rslf_f2c_run_withheld(run_, level, &n), "rslf_f2c_run_withheld");
        return n;
    }
    // After run() with set_peaks(true): a level's four planes; the fused peaks at the finest size -- for every pixel of the
    // fused map the peaks of the pixel of the deciding level it was taken from (the NEAREST pixel down the fusion's mask
    // chain, not the bilinear blend and median the fused disparity went through); and the level that decided it (255: none).
    Peaks get_level_peaks(int level) const
    {
        detail::require(run_ != nullptr && peaks_held_, "get_level_peaks: the peak planes are held by a kept run made with set_peaks(true)");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_level_peaks: the level is not in the pyramid");
        return copy_peaks(level, (size_t)dim_s_ * dims_[level].first * dims_[level].second, RSLF_F2C_PLANE_PK_IDX);
    }
    Peaks get_fused_peaks() const
    {
        detail::require(run_ != nullptr && peaks_held_, "get_fused_peaks: the peak planes are held by a kept run made with set_peaks(true)");
        return copy_peaks(0, (size_t)dim_s_ * dim_v_ * dim_u_, RSLF_F2C_PLANE_FUSED_PK_IDX);
    }
    std::vector<uint8_t> get_fused_level() const
    {
        detail::require(run_ != nullptr && peaks_held_, "get_fused_level: the peak planes are held by a kept run made with set_peaks(true)");
        std::vector<uint8_t> out((size_t)dim_s_ * dim_v_ * dim_u_);
        check(rslf_f2c_run_copy(run_, 0, RSLF_F2C_PLANE_FUSED_LEVEL, out.data(), 1, nullptr), "rslf_f2c_run_copy");
        return out;
    }
    // Not in the reference: after a run() that followed keep_on_device, the cross-view consistency of a kept plane pair, read
    // in place on the device (rslf_f2c_run_consistency_host, rslf_hip.h): the fused map and its validity (fused_result, which
    // needs level 0) or a level's disparities and validity, with the slope factor the level's sweep ran with.  tol < 0: one
    // step of the hypothesis grid.  -> planes [S][V_level][U_level].  An object built on a MultiContext has no kept run.
    Consistency get_consistency(Context& on, int level = 0, bool fused_result = true, float tol = -1.f, int radius = 0,
                                int min_agree = 0) const
    {
        detail::require(run_ != nullptr, "get_consistency reads a kept run's planes on the device: call keep_on_device before run()");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_consistency: the level is not in the pyramid");
        Consistency out;
        const rslf_view_counts counts = detail::consistency_planes(out, (size_t)dim_s_ * dims_[level].first * dims_[level].second);
        check(rslf_f2c_run_consistency_host(run_, on.get(), level, fused_result ? 1 : 0,
                                            tol < 0.f ? detail::grid_step(d_min_, d_max_, dim_d_) : tol, radius, min_agree, &counts,
                                            out.fused.data(), out.valid.data()),
              "rslf_f2c_run_consistency_host");
        return out;
    }
    Consistency get_consistency(int level = 0, bool fused_result = true, float tol = -1.f, int radius = 0, int min_agree = 0) const
    {
        return get_consistency(detail::own(ctx_), level, fused_result, tol, radius, min_agree);
    }
    // Not in the reference: after a run() that followed keep_on_device, the view warp of a kept plane pair, read in place on the
    // device (rslf_f2c_run_view_warp_host, rslf_hip.h): the fused map and its validity (fused_result, which needs level 0) or
    // a level's disparities and validity, with the slope factor the level's sweep ran with and the level's kept volume -- a
    // run kept without its volumes refuses colour.  -> planes [1][V_level][U_level].
    Warp get_warped_view(Context& on, float target, int level = 0, bool fused_result = true, int exclude = -1, int radius = 0,
                         int nearer = 1, bool colour = true) const
    {
        detail::require(run_ != nullptr, "get_warped_view reads a kept run's planes on the device: call keep_on_device before run()");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_warped_view: the level is not in the pyramid");
        Warp out;
        const rslf_view_warp_out planes = detail::warp_planes(out, (size_t)dims_[level].first * dims_[level].second, CHANNELS, colour);
        check(rslf_f2c_run_view_warp_host(run_, on.get(), level, fused_result ? 1 : 0, &target, &exclude, 1, radius, nearer, &planes),
              "rslf_f2c_run_view_warp_host");
        return out;
    }
    Warp get_warped_view(float target, int level = 0, bool fused_result = true, int exclude = -1, int radius = 0, int nearer = 1,
                         bool colour = true) const
    {
        return get_warped_view(detail::own(ctx_), target, level, fused_result, exclude, radius, nearer, colour);
    }
    // ... and the novel view of a kept plane pair (rslf_f2c_run_novel_view_host): a finished image of `target`, with the
    // level's kept volume -- a run kept without its volumes refuses colour.  -> planes [V_level][U_level].
    NovelView get_novel_view(Context& on, float target, int level = 0, bool fused_result = true, int exclude = -1,
                             const NovelViewOptions& options = NovelViewOptions(), bool colour = true) const
    {
        detail::require(run_ != nullptr, "get_novel_view reads a kept run's planes on the device: call keep_on_device before run()");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_novel_view: the level is not in the pyramid");
        NovelView out;
        const rslf_novel_view_out planes = detail::novel_planes(out, (size_t)dims_[level].first * dims_[level].second, CHANNELS, colour);
        const rslf_novel_view_params params = detail::novel_params(options, options.tol < 0.f ? detail::grid_step(d_min_, d_max_, dim_d_) : 0.f);
        check(rslf_f2c_run_novel_view_host(run_, on.get(), level, fused_result ? 1 : 0, &target, &exclude, 1, &params, &planes),
              "rslf_f2c_run_novel_view_host");
        return out;
    }
    NovelView get_novel_view(float target, int level = 0, bool fused_result = true, int exclude = -1,
                             const NovelViewOptions& options = NovelViewOptions(), bool colour = true) const
    {
        return get_novel_view(detail::own(ctx_), target, level, fused_result, exclude, options, colour);
    }
    ViewPrediction get_view_prediction(Context& on, int level = 0, bool fused_result = true, std::vector<int> views = std::vector<int>(),
                                       int radius = 0, int nearer = 1) const
    {
        detail::require(run_ != nullptr, "get_view_prediction reads a kept run's planes on the device: call keep_on_device before run()");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_view_prediction: the level is not in the pyramid");
        const std::vector<float> targets = detail::prediction_targets(views, dim_s_);
        ViewPrediction out;
        const rslf_view_warp_out planes = detail::prediction_planes(out, (int)views.size(), dims_[level].first, dims_[level].second);
        check(rslf_f2c_run_view_warp_host(run_, on.get(), level, fused_result ? 1 : 0, targets.data(), views.data(), (int)views.size(), radius,
                                          nearer, &planes),
              "rslf_f2c_run_view_warp_host");
        detail::prediction_finish(out, (int)views.size(), dims_[level].first, dims_[level].second);
        return out;
    }
    ViewPrediction get_view_prediction(int level = 0, bool fused_result = true, std::vector<int> views = std::vector<int>(), int radius = 0,
                                       int nearer = 1) const
    {
        return get_view_prediction(detail::own(ctx_), level, fused_result, views, radius, nearer);
    }
    // Not in the reference, to be called before run() and after keep_on_device: validity by cross-view consistency
    // (rslf_f2c_run_host_cs, rslf_hip.h).  After a level's sweep, validity rule and uniqueness ratio, a pixel that is still
    // valid becomes invalid unless agree >= min(seen, min_agree) among the other views (radius > 0: |t - s| <= radius), so the
    // next level's ranges and the fusion leave it to a coarser level.  min_agree = 0 switches it off; tol < 0: one step of
    // the hypothesis grid.  Needs no peaks.  One device only: throws on a MultiContext.
    void set_consistency_gate(int min_agree, float tol = -1.f, int radius = 0)
    {
        if (multi_)
            throw std::invalid_argument("set_consistency_gate: this object was built on a MultiContext: the pyramid's consistency gate is built for one context");
        detail::require(keep_, "FineToCoarse: the consistency gate belongs to a kept run: call keep_on_device first");
        detail::require(min_agree >= 0, "consistency gate: min_agree is 0 (off) or a count of agreeing views >= 1");
        if (min_agree > 0 && tol < 0.f)
            tol = detail::grid_step(d_min_, d_max_, dim_d_);
        detail::require(min_agree == 0 || (tol >= 0.f && tol <= 3.402823466e+38f), "consistency gate: tol is a finite tolerance >= 0");
        gate_min_agree_ = min_agree;
        gate_tol_ = min_agree > 0 ? tol : 0.f;
        gate_radius_ = min_agree > 0 ? radius : 0;
    }
    int get_consistency_min_agree() const { return gate_min_agree_; }
    // After run() with the gate set: the pixels the gate made invalid on a level (0 on a level accepted whole), and the
    // gate's own counts at gate time -- agree and seen [S][V_level][U_level], the other planes of the Consistency empty.
    unsigned long long get_inconsistent(int level) const
    {
        detail::require(run_ != nullptr, "get_inconsistent: the counts are held by a kept run: keep_on_device, then run()");
        unsigned long long n = 0;
        check(rslf_f2c_run_inconsistent(run_, level, &n), "rslf_f2c_run_inconsistent");
        return n;
    }
    Consistency get_gate_counts(int level) const
    {
        detail::require(run_ != nullptr && gate_held_, "get_gate_counts: the planes are held by a kept run made with set_consistency_gate");
        detail::require(level >= 0 && level < (int)dims_.size(), "get_gate_counts: the level is not in the pyramid");
        Consistency out;
        const size_t n = (size_t)dim_s_ * dims_[level].first * dims_[level].second;
        out.agree.resize(n), out.seen.resize(n);
        check(rslf_f2c_run_copy(run_, level, RSLF_F2C_PLANE_CS_AGREE, out.agree.data(), 1, nullptr), "rslf_f2c_run_copy");
        check(rslf_f2c_run_copy(run_, level, RSLF_F2C_PLANE_CS_SEEN, out.seen.data(), 1, nullptr), "rslf_f2c_run_copy");
        return out;
    }
    ~FineToCoarse() { rslf_f2c_run_destroy(run_); }
    FineToCoarse(const FineToCoarse&) = delete;
    FineToCoarse& operator=(const FineToCoarse&) = delete;
    void run()
    {
        const rslf_params p = m_parameters.to_c();
        if (keep_) {
            run_kept(p);
            return;
        }
        const size_t n = (size_t)dim_s_ * dim_v_ * dim_u_;
        out_map_s_v_u_.assign(n, 0.f);
        out_validity_s_v_u_.assign(n, 0);
        if (line_mode_ >= 0 || subgrid_) {
            run_levels(p);
            return;
        }
        if (multi_) {   // (set_derivative_channels refused a weight)
            if (type_ == InputType::U16)   // ushort arithmetic through the pyramid
                check(rslf_multi_fine_to_coarse_run_host_u16(multi_->get(), (const uint16_t* const*)epis_.data(), dim_v_, dim_s_, dim_u_,
                                                             CHANNELS, stride_, d_min_, d_max_, dim_d_, scale_, &p, max_pyr_depth_,
                                                             accept_all_ ? 1 : 0, out_map_s_v_u_.data(), out_validity_s_v_u_.data(),
                                                             &n_levels_, &stats),
                      "rslf_multi_fine_to_coarse_run_host_u16");
            else
                check(rslf_multi_fine_to_coarse_run_host(multi_->get(), epis_.data(), type_ == InputType::U8 ? 1 : 0, dim_v_, dim_s_, dim_u_,
                                                         CHANNELS, stride_, d_min_, d_max_, dim_d_, scale_, &p, max_pyr_depth_,
                                                         accept_all_ ? 1 : 0, out_map_s_v_u_.data(), out_validity_s_v_u_.data(), &n_levels_,
                                                         &stats),
                      "rslf_multi_fine_to_coarse_run_host");
            return;
        }
        // the family's widest entry, which takes any element type: no mode, no levels out
        check(rslf_fine_to_coarse_run_host_eq(ctx_->get(), epis_.data(), elem(), dim_v_, dim_s_, dim_u_, CHANNELS, stride_, d_min_, d_max_,
                                              dim_d_, scale_, &p, max_pyr_depth_, accept_all_ ? 1 : 0, out_map_s_v_u_.data(),
                                              out_validity_s_v_u_.data(), &n_levels_, &stats, RSLF_LINE_CONF_OFF, nullptr, 0,
                                              derivative_weight_, level_dilation_, level_dilation_kind_, equalize_mode_, equalize_ref_view_,
                                              equalize_joint_, equalize_max_gain_),
              "rslf_fine_to_coarse_run_host_eq");
    }
    void get_results(std::vector<float>& out_map_s_v_u, std::vector<uint8_t>& out_validity_s_v_u) const
    {
        if (run_) {   // a kept run: the fused planes come from the device
            const size_t n = (size_t)dim_s_ * dim_v_ * dim_u_;
            out_map_s_v_u.resize(n);
            out_validity_s_v_u.resize(n);
            check(rslf_f2c_run_copy(run_, 0, RSLF_F2C_PLANE_FUSED_MAP, out_map_s_v_u.data(), 1, nullptr), "rslf_f2c_run_copy");
            check(rslf_f2c_run_copy(run_, 0, RSLF_F2C_PLANE_FUSED_VALID, out_validity_s_v_u.data(), 1, nullptr), "rslf_f2c_run_copy");
            return;
        }
        out_map_s_v_u = out_map_s_v_u_;
        out_validity_s_v_u = out_validity_s_v_u_;
    }
    // rslf_fine_to_coarse.hpp:325-378: the fused disparities of every view through ONE converter, fitted on the fused plane
    // (int)std::round(S / 2.0) (saturate: 2 % / 98 % quantiles, else min and mean + 12 std), colour-mapped, black where the
    // fused validity is 0 and, with par_cut_shadows, where the finest level's radiance is in shadow -> [S][V][U][3].
    // S = 1 throws: the reference's index is then S itself.  The shadow cut reads the EPIs the constructor was given
    // (into a volume of its own, as the constructor's copy would): their buffers must outlive this call.
    std::vector<uint8_t> get_coloured_depth_maps(Context& on, const uint8_t* lut_bgr, bool saturate = true) const
    {
        if (run_) {   // rendered on the device from the kept planes; the shadow cut reads the kept level-0 volume
            std::vector<uint8_t> out((size_t)dim_s_ * dim_v_ * dim_u_ * 3);
            check(rslf_f2c_run_render_depth_maps_host(run_, on.get(), saturate ? 1 : 0, lut_bgr, out.data()), "rslf_f2c_run_render_depth_maps_host");
            return out;
        }
        int mid = 0;
        check(rslf_render_centre_index(dim_s_, &mid), "get_coloured_depth_maps");
        detail::require(!out_map_s_v_u_.empty(), "the getters show the results of run(): call it first");
        struct Shadow {   // the finest level's radiance on the device, for the time of the call
            rslf_volume* vol;
            Shadow() : vol(nullptr) {}
            ~Shadow() { rslf_volume_destroy(vol); }
        } shadow;
        if (m_parameters.par_cut_shadows) {
            check(rslf_volume_create(on.get(), dim_v_, dim_s_, dim_u_, CHANNELS, &shadow.vol), "rslf_volume_create");
            detail::upload_epis(shadow.vol, type_, epis_.data(), stride_, scale_);
        }
        return detail::render_planes(on.get(), out_map_s_v_u_, 0, out_validity_s_v_u_.data(), dim_s_, (size_t)dim_v_ * dim_u_, dim_v_, dim_u_,
                                     (size_t)dim_u_, saturate ? RSLF_FIT_QUANTILE : RSLF_FIT_MEANSTD, mid, RSLF_RENDER_AFFINE, lut_bgr,
                                     shadow.vol, m_parameters.par_shadow_level);
    }
    std::vector<uint8_t> get_coloured_depth_maps(const uint8_t* lut_bgr, bool saturate = true) const
    {
        return get_coloured_depth_maps(detail::own(ctx_), lut_bgr, saturate);
    }
    int pyramid_depth() const { return n_levels_; }
    // After a run() that followed set_line_confidence_mode or keep_on_device: the level sizes (V_p, U_p), finest first, and
    // every level's [S][V_p][U_p] disparities, validity mask and line confidence (empty planes with RSLF_LINE_CONF_OFF).
    // A kept run copies a kind of plane out of the device when it is first asked for, and has the disparity confidence too.
    const std::vector<std::pair<int, int> >& pyramid_dims() const { return dims_; }
    const std::vector<std::vector<float> >& get_depths_pyr() const { return kept_pyr(depths_pyr_, RSLF_F2C_PLANE_DEPTH); }
    const std::vector<std::vector<uint8_t> >& get_validity_pyr() const { return kept_pyr(validity_pyr_, RSLF_F2C_PLANE_VALID); }
    const std::vector<std::vector<float> >& get_line_confidence_pyr() const
    {
        return (run_ && line_mode_ <= RSLF_LINE_CONF_OFF) ? line_confidence_pyr_ : kept_pyr(line_confidence_pyr_, RSLF_F2C_PLANE_CL);
    }
    const std::vector<std::vector<float> >& get_disp_confidence_pyr() const
    {
        detail::require(run_ != nullptr, "get_disp_confidence_pyr: the disparity confidence of every level is held by a kept run (keep_on_device)");
        return kept_pyr(disp_confidence_pyr_, RSLF_F2C_PLANE_CD);
    }
    // rslf_fine_to_coarse.hpp:491-519: view s (-1: (int)std::round(S / 2.0)) of every level, finest first, through the
    // converter fitted on level 0's plane before any masking; black outside each level's validity; no shadow cut ->
    // one [V_p][U_p][3] picture per level.  Throws where the reference's index runs off the end (S = 1).
    std::vector<std::vector<uint8_t> > get_coloured_depth_pyr(Context& on, int s, const uint8_t* lut_bgr, bool saturate = true) const
    {
        if (run_)
            return kept_pictures(on, s, lut_bgr, saturate, false);
        detail::require(!depths_pyr_.empty(), "get_coloured_depth_pyr shows the levels of a run() after set_line_confidence_mode or keep_on_device");
        if (s == -1)
            check(rslf_render_centre_index(dim_s_, &s), "get_coloured_depth_pyr");
        detail::require(s >= 0 && s < dim_s_, "get_coloured_depth_pyr: the view is not below dim_s");
        std::vector<std::vector<uint8_t> > out(dims_.size());
        double mm[2] = {0.0, 0.0};
        for (size_t l = 0; l < dims_.size(); l++) {
            const int rows = dims_[l].first, cols = dims_[l].second;
            const size_t o = (size_t)s * rows * cols;
            out[l].resize((size_t)rows * cols * 3);
            check(rslf_render_planes_host(on.get(), depths_pyr_[l].data() + o, 1, 0, rows, cols, (size_t)cols, validity_pyr_[l].data() + o,
                                          l == 0 ? (saturate ? RSLF_FIT_QUANTILE : RSLF_FIT_MEANSTD) : RSLF_FIT_GIVEN, -1, 0,
                                          RSLF_RENDER_AFFINE, lut_bgr, RSLF_MASK_BLACK, nullptr, RSLF_SLICE_VIEW, 0, 0.f, out[l].data(), mm),
                  "rslf_render_planes_host");
        }
        return out;
    }
    std::vector<std::vector<uint8_t> > get_coloured_depth_pyr(int s, const uint8_t* lut_bgr, bool saturate = true) const
    {
        return get_coloured_depth_pyr(detail::own(ctx_), s, lut_bgr, saturate);
    }
    // rslf_fine_to_coarse.hpp:432-488, of a kept run: the S x U_p slice of every level at scanline
    // (int)std::round(1.0 * v * V_p / V_0) (v = -1: (int)std::round(V_0 / 2.0)), finest first; invalid pixels count as 0 in the
    // fit (level 0) and in the render; with par_cut_shadows the shadow cut against the level's own kept volume -> one
    // [S][U_p][3] picture per level.  Throws where the reference's row index reaches V_p.
    std::vector<std::vector<uint8_t> > get_coloured_epi_pyr(Context& on, int v, const uint8_t* lut_bgr, bool saturate = true) const
    {
        detail::require(run_ != nullptr, "get_coloured_epi_pyr reads every level's planes and volume on the device: call keep_on_device before run()");
        return kept_pictures(on, v, lut_bgr, saturate, true);
    }
    std::vector<std::vector<uint8_t> > get_coloured_epi_pyr(int v, const uint8_t* lut_bgr, bool saturate = true) const
    {
        return get_coloured_epi_pyr(detail::own(ctx_), v, lut_bgr, saturate);
    }
    rslf_stats stats;

private:
    FineToCoarse(Context* ctx, MultiContext* multi, const void* const* epis, InputType type, int dim_v, int dim_s, int dim_u,
                 size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor, const Depth1DParameters& parameters,
                 int max_pyr_depth, bool accept_all_last_scale)
        : ctx_(ctx), multi_(multi), epis_(epis, epis + dim_v), type_(type), dim_v_(dim_v), dim_s_(dim_s), dim_u_(dim_u),
          stride_(row_stride_bytes), d_min_(d_min), d_max_(d_max), dim_d_(dim_d), scale_(epi_scale_factor),
          m_parameters(parameters), max_pyr_depth_(max_pyr_depth), accept_all_(accept_all_last_scale), n_levels_(0), line_mode_(-1),
          keep_(false), keep_volumes_(true), validity_rule_(RSLF_F2C_VALID_COMPAT), run_(nullptr)
    {
        stats = rslf_stats();
    }
    // run() through rslf_f2c_run_host: the run stays on the device, this object owns the handle
    void run_kept(const rslf_params& p)
    {
        rslf_f2c_run_destroy(run_);
        run_ = nullptr;
        out_map_s_v_u_.clear();
        out_validity_s_v_u_.clear();
        depths_pyr_.clear();
        validity_pyr_.clear();
        line_confidence_pyr_.clear();
        disp_confidence_pyr_.clear();
        dims_.clear();
        peaks_held_ = false;
        detail::require(peaks_ || uniqueness_ == 0.f, "FineToCoarse: the uniqueness ratio reads the peak planes: call set_peaks(true)");
        detail::require(peaks_ || propagation_ratio_ == 0.f, "FineToCoarse: the propagation ratio reads the peak planes: call set_peaks(true)");
        gate_held_ = false;
        // the family's widest entry: what is off goes in neutral (0), and the run is the narrower entry's (rslf_hip.h)
        check(rslf_f2c_run_host_eq(ctx_->get(), epis_.data(), elem(), dim_v_, dim_s_, dim_u_, CHANNELS, stride_, d_min_, d_max_, dim_d_, scale_,
                                   &p, max_pyr_depth_, accept_all_ ? 1 : 0, line_mode_ < 0 ? RSLF_LINE_CONF_OFF : line_mode_, validity_rule_,
                                   keep_volumes_ ? 1 : 0, &run_, &stats, subgrid_ ? 1 : 0, peaks_ ? 1 : 0, uniqueness_, propagation_ratio_,
                                   gate_tol_, gate_radius_, gate_min_agree_, derivative_weight_, level_dilation_, level_dilation_kind_,
                                   equalize_mode_, equalize_ref_view_, equalize_joint_, equalize_max_gain_),
              "rslf_f2c_run_host_eq");
        peaks_held_ = peaks_;
        gate_held_ = gate_min_agree_ > 0;
        rslf_f2c_run_desc d;
        check(rslf_f2c_run_describe(run_, &d), "rslf_f2c_run_describe");
        n_levels_ = d.n_levels;
        for (int l = 0; l < d.n_levels; l++)
            dims_.push_back(std::make_pair(d.V[l], d.U[l]));
    }
    // four peak planes of a kept run, RSLF_F2C_PLANE_PK_* or _FUSED_PK_* counted from `first`
    Peaks copy_peaks(int level, size_t n, int first) const
    {
        Peaks out;
        out.idx.resize(n), out.score.resize(n), out.runner_idx.resize(n), out.runner_score.resize(n);
        check(rslf_f2c_run_copy(run_, level, first, out.idx.data(), 1, nullptr), "rslf_f2c_run_copy");
        check(rslf_f2c_run_copy(run_, level, first + 1, out.score.data(), 1, nullptr), "rslf_f2c_run_copy");
        check(rslf_f2c_run_copy(run_, level, first + 2, out.runner_idx.data(), 1, nullptr), "rslf_f2c_run_copy");
        check(rslf_f2c_run_copy(run_, level, first + 3, out.runner_score.data(), 1, nullptr), "rslf_f2c_run_copy");
        return out;
    }
    // one kind of plane of every level of a kept run, copied out when first asked for; without a kept run, what run() left
    template <typename T>
    const std::vector<std::vector<T> >& kept_pyr(std::vector<std::vector<T> >& pyr, int which) const
    {
        if (!run_ || !pyr.empty())
            return pyr;
        std::vector<std::vector<T> > planes(dims_.size());
        for (size_t l = 0; l < dims_.size(); l++) {
            planes[l].resize((size_t)dim_s_ * dims_[l].first * dims_[l].second);
            check(rslf_f2c_run_copy(run_, (int)l, which, planes[l].data(), 1, nullptr), "rslf_f2c_run_copy");
        }
        pyr.swap(planes);
        return pyr;
    }
    // get_coloured_depth_pyr / get_coloured_epi_pyr of a kept run, one picture per level
    std::vector<std::vector<uint8_t> > kept_pictures(Context& on, int index, const uint8_t* lut_bgr, bool saturate, bool epi) const
    {
        std::vector<std::vector<uint8_t> > out(dims_.size());
        std::vector<uint8_t*> ptrs(dims_.size());
        for (size_t l = 0; l < dims_.size(); l++) {
            out[l].resize((size_t)(epi ? dim_s_ : dims_[l].first) * dims_[l].second * 3);
            ptrs[l] = out[l].data();
        }
        if (epi)
            check(rslf_f2c_run_render_epi_pyr_host(run_, on.get(), index, saturate ? 1 : 0, lut_bgr, ptrs.data()), "rslf_f2c_run_render_epi_pyr_host");
        else
            check(rslf_f2c_run_render_depth_pyr_host(run_, on.get(), index, saturate ? 1 : 0, lut_bgr, ptrs.data()), "rslf_f2c_run_render_depth_pyr_host");
        return out;
    }
    // run() through rslf_fine_to_coarse_run_host_sub, every level's planes kept
    void run_levels(const rslf_params& p)
    {
        const int mode = line_mode_ < 0 ? RSLF_LINE_CONF_OFF : line_mode_;   // (set_subgrid alone leaves the line mode unset)
        int P = 0;
        check(rslf_f2c_pyramid_dims(dim_v_, dim_u_, max_pyr_depth_, nullptr, nullptr, 0, &P), "rslf_f2c_pyramid_dims");
        std::vector<int> Vp(P), Up(P);
        check(rslf_f2c_pyramid_dims(dim_v_, dim_u_, max_pyr_depth_, Vp.data(), Up.data(), P, &P), "rslf_f2c_pyramid_dims");
        dims_.clear();
        depths_pyr_.assign(P, std::vector<float>());
        validity_pyr_.assign(P, std::vector<uint8_t>());
        line_confidence_pyr_.assign(P, std::vector<float>());
        std::vector<float*> hd(P), hl(P);
        std::vector<uint8_t*> hv(P);
        for (int l = 0; l < P; l++) {
            const size_t nl = (size_t)dim_s_ * Vp[l] * Up[l];
            dims_.push_back(std::make_pair(Vp[l], Up[l]));
            depths_pyr_[l].assign(nl, 0.f);
            validity_pyr_[l].assign(nl, 0);
            if (mode != RSLF_LINE_CONF_OFF)
                line_confidence_pyr_[l].assign(nl, 0.f);
            hd[l] = depths_pyr_[l].data();
            hv[l] = validity_pyr_[l].data();
            hl[l] = mode != RSLF_LINE_CONF_OFF ? line_confidence_pyr_[l].data() : nullptr;
        }
        rslf_f2c_levels_out lo;
        lo.capacity = P;
        lo.h_depth_svu = hd.data();
        lo.h_valid_svu = hv.data();
        lo.h_Cl_svu = hl.data();
        lo.h_Ce_svu = nullptr;
        // the family's widest entry, which takes any element type
        check(rslf_fine_to_coarse_run_host_eq(ctx_->get(), epis_.data(), elem(), dim_v_, dim_s_, dim_u_, CHANNELS, stride_, d_min_, d_max_,
                                              dim_d_, scale_, &p, max_pyr_depth_, accept_all_ ? 1 : 0, out_map_s_v_u_.data(),
                                              out_validity_s_v_u_.data(), &n_levels_, &stats, mode, &lo, subgrid_ ? 1 : 0, derivative_weight_,
                                              level_dilation_, level_dilation_kind_, equalize_mode_, equalize_ref_view_, equalize_joint_,
                                              equalize_max_gain_),
              "rslf_fine_to_coarse_run_host_eq");
    }
    int elem() const { return type_ == InputType::U8 ? RSLF_ELEM_U8 : type_ == InputType::U16 ? RSLF_ELEM_U16 : RSLF_ELEM_F32; }
#ifdef RSLFX_HAVE_OPENCV
    FineToCoarse(Context* ctx, MultiContext* multi, const detail::MatInput& in, float d_min, float d_max, int dim_d,
                 float epi_scale_factor, const Depth1DParameters& parameters, int max_pyr_depth, bool accept_all_last_scale)
        : FineToCoarse(ctx, multi, in.ptrs.data(), in.type, in.V, in.S, in.U, in.stride, d_min, d_max, dim_d, epi_scale_factor,
                       parameters, max_pyr_depth, accept_all_last_scale)
    {
    }
#endif
    Context* ctx_;
    MultiContext* multi_;
    std::vector<const void*> epis_;
    InputType type_;
    int dim_v_, dim_s_, dim_u_;
    size_t stride_;
    float d_min_, d_max_;
    int dim_d_;
    float scale_;
    const Depth1DParameters m_parameters;
    int max_pyr_depth_;
    bool accept_all_;
    int n_levels_;
    int line_mode_;   // -1: set_line_confidence_mode was not called
    std::vector<float> out_map_s_v_u_;
    std::vector<uint8_t> out_validity_s_v_u_;
    std::vector<std::pair<int, int> > dims_;
    mutable std::vector<std::vector<float> > depths_pyr_, line_confidence_pyr_, disp_confidence_pyr_;   // (filled by the const getters of a kept run)
    mutable std::vector<std::vector<uint8_t> > validity_pyr_;
    bool keep_, keep_volumes_;   // keep_on_device
    bool subgrid_ = false;       // set_subgrid
    bool peaks_ = false;         // set_peaks
    float uniqueness_ = 0.f;     // set_uniqueness_ratio
    float propagation_ratio_ = 0.f;   // set_propagation_ratio
    bool peaks_held_ = false;    // the kept run was made with peaks
    int gate_min_agree_ = 0, gate_radius_ = 0;   // set_consistency_gate
    float gate_tol_ = 0.f;
    bool gate_held_ = false;     // the kept run was made with the consistency gate
    float derivative_weight_ = 0.f;   // set_derivative_channels
    int level_dilation_ = 1, level_dilation_kind_ = RSLF_DILATE_CUBIC;   // set_level_dilation
    int equalize_mode_ = 0, equalize_ref_view_ = 0, equalize_joint_ = 0;  // set_equalize_views
    float equalize_max_gain_ = 4.f;
    int validity_rule_;
    rslf_f2c_run* run_;          // the kept run, owned
};

typedef Depth1DComputer_pile<1> Depth1DComputer_pile_1ch;   // dc.hpp:149
typedef Depth1DComputer_pile<3> Depth1DComputer_pile_3ch;   // dc.hpp:154

}  // namespace rslfx

#endif  // RSLF_HIP_HPP
