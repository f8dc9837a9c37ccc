// CV_16U Mats into the three cv::Mat-facing classes of include/rslf_hip.hpp, compiled with -fsyntax-only against the
// declaration-only mock in tests/cpp/opencv_mock with -DCV_16U=2 (the mock itself defines no CV_16U; every OpenCV does,
// as a macro, and the wrapper's 16U branch is guarded by it).  tests/test_u16_cpu.py.
#include "rslf_hip.hpp"
#ifndef RSLFX_HAVE_OPENCV
#error "the mock <opencv2/core/core.hpp> is not on the include path"
#endif
#ifndef CV_16U
#error "compile with -DCV_16U=2"
#endif

void use_u16(rslfx::Context& ctx, rslfx::MultiContext& multi, const std::vector<cv::Mat>& epis_16u)
{
    rslfx::InputType type = rslfx::InputType::F32;
    const std::vector<const void*> ptrs = rslfx::Depth1DComputer_pile<1>::mat_pointers(epis_16u, type);
    (void)ptrs;
    rslfx::Depth1DComputer_pile<1> a(ctx, epis_16u, -1.f, 2.f, 16);
    a.run();
    rslfx::Depth1DComputer_pile<3> b(multi, epis_16u, -1.f, 2.f, 16, -1, 4095.f);
    b.run();
    rslfx::Depth2DComputer<1> c(ctx, epis_16u, -1.f, 2.f, 9);
    c.run();
    rslfx::Depth2DComputer<3> d(multi, epis_16u, -1.f, 2.f, 9, -1.f);
    d.run();
    rslfx::FineToCoarse<1> e(ctx, epis_16u, -1.f, 1.f, 9);
    e.run();
    rslfx::FineToCoarse<3> f(multi, epis_16u, -1.f, 1.f, 9, -1.f, rslfx::Depth1DParameters::get_default(), -1, true);
    f.run();
}
