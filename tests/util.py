"""Shared helpers for the parity tests."""
from __future__ import annotations

import numpy as np

# BASELINE.md §7 / north_star: argmax indices bit-exact, confidences within 1e-5
TOL = 1e-5


def assert_pile_parity(got: dict, ref, *, exact_float: bool = True, label: str = ""):
    """got: dict of numpy planes from the HIP path; ref: oracle.PileResult.

    Integer / mask planes must match bit for bit.  Float planes are asserted
    within TOL (the bar north_star states) and, when exact_float, additionally
    required to be bit-identical -- the HIP kernels perform the same IEEE
    operations in the same order as the oracle, so any difference is a bug.
    """
    def eq(name, a, b):
        assert a.shape == b.shape, (label, name, a.shape, b.shape)
        af, bf = a.reshape(-1), b.reshape(-1)
        differ = af != bf
        if af.dtype.kind == "f":   # a NaN in the same place on both sides is agreement (NaN inputs propagate into C_e)
            differ &= ~(np.isnan(af) & np.isnan(bf))
        bad = np.flatnonzero(differ)
        assert bad.size == 0, "%s %s: %d mismatches, first at %s: got %r want %r" % (
            label, name, bad.size, np.unravel_index(bad[0], a.shape), a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])

    eq("edge_mask", got["edge_mask"], ref.edge_mask)
    eq("depth_idx", got["depth_idx"], ref.depth_idx)
    for name, a, b in (("edge_confidence", got["edge_confidence"], ref.edge_confidence),
                       ("score", got["score"], ref.score),
                       ("disp_confidence", got["disp_confidence"], ref.disp_confidence),
                       ("rbar", got["rbar"], ref.rbar),
                       ("depth_raw", got["depth_raw"], ref.depth_raw),
                       ("depth", got["depth"], ref.depth)):
        assert a.shape == b.shape, (label, name, a.shape, b.shape)
        with np.errstate(invalid="ignore"):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
        d = np.where(np.isinf(a) & (a == b), 0.0, d)
        err = d.max() if a.size else 0.0
        assert err <= TOL, "%s %s: max abs err %g > %g" % (label, name, err, TOL)
        if exact_float and name != "disp_confidence":
            eq(name, a, b)


def native_fine_to_coarse(epis, d_min: float, d_max: float, dim_d: int, epi_scale_factor: float = -1.0, max_pyr_depth: int = -1,
                          accept_all_last_scale: bool = True):
    """The one-context native level loop (rslf_fine_to_coarse_run_host) on the default context of cuda:0, from a list of
    float32 or uint8 host EPIs (padded rows go up in place, depth.host_rows): (out_map [S,V,U] f32, out_validity [S,V,U] u8, levels, rslf_stats)."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    keep, ptrs, dt, V, S, U, C_, stride = rs.host_epis(epis, stride=True)
    assert dt in (np.float32, np.uint8), dt
    out_map, out_valid = np.empty((S, V, U), np.float32), np.empty((S, V, U), np.uint8)
    p = rs.Depth1DParameters().to_c()
    st, nl = _lib.RslfStats(), C.c_int()
    _lib.check(_lib.lib().rslf_fine_to_coarse_run_host(
        rs.default_context(0)._h, ptrs, int(dt == np.uint8), V, S, U, C_, stride, float(d_min), float(d_max), int(dim_d),
        float(epi_scale_factor), C.byref(p), int(max_pyr_depth), int(accept_all_last_scale), out_map.ctypes.data_as(C.c_void_p),
        out_valid.ctypes.data_as(C.c_void_p), C.byref(nl), C.byref(st)), "rslf_fine_to_coarse_run_host")
    return out_map, out_valid, int(nl.value), st
