"""EVERY instantiation of the weight-sharing predictive kernels on the MI355X, against the fp64 definition.

``quadform_conv_planes_kernel<CT, OCC, SUB>``, ``quadform_conv_kernel<CT, MODE, ARITH>``, ``diag_ggn_shared_kernel<CT, B6>``
and ``quadform_shared_grid_kernel<CT, MODE, ARITH>`` (csrc/lk_quadconv.hip, lk_grid.hip) are templates; the launchers pick one
of several dozen compiled kernels from the number of outputs, the layer width and the map size, each with its own register
budget, LDS ring depth, counted waits and padding of staged outputs.  The older tests launch what ResNet-18 with ten classes
picks.  Here one case per (family, variant, number of outputs) of tests/quad_fixtures.py ``CASES``: every case first asks
``lk_quadform_shared_variant`` that its shape launches the kernel its id names (tests/test_quad_fixtures.py proves on the CPU
that the table reaches all of them), then holds it to

    |got - want| <= 1e-4 |want| + 1e-6 max|want|        element-wise, max per sample / per (grid point, sample) / per vector

on correlated, differently scaled outputs (every pair sum a distinct large number), post-ReLU inputs over five decades of
per-sample magnitude, and both a flat and a clamped ten-decade KFAC spectrum.  Replaces, for weight-sharing layers,
KronDecomposed._bmm / inv_square_form under KronLaplace.functional_variance (laplace/utils/matrix.py:406-461,
baselaplace.py:1834-1835), DiagLaplace.functional_variance (baselaplace.py:2113-2115), GGNInterface.diag
(curvature.py:413-433) and the prior-precision grid search (baselaplace.py:487-561).  Measured ratios:
profiles/quadform_instances.md."""
from types import SimpleNamespace

import pytest
import torch

from tests import quad_fixtures as qf
from tests.parity_log import record_error

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4096  # guard floats on either side of an output


def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


def params(family):
    rows = qf.CASES[family]
    return pytest.mark.parametrize("row", rows, ids=[qf.row_id(r) for r in rows])


def held(got, want, scope, what):
    """the tolerance of the file's docstring; the ratio goes to the parity log under the test's id"""
    ratio = record_error(qf.tolerance_ratio(got, want, scope))
    print(f"{what}: |err| / tolerance = {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: |err| / tolerance = {ratio:.3g}"


def routes_agree(a, b, lead, tol, what):
    """route against route: of the largest entry under each of the ``lead`` leading indices (sample / grid point and sample)"""
    a, b = a.double().flatten(lead), b.double().flatten(lead)
    err = record_error(((a - b).abs().amax(-1) / b.abs().amax(-1).clamp_min(1e-300)).max().item(), tag="routes")
    assert err < tol, f"{what}: {err:.3g}"


def reference_device(ops):
    """the fp64 reference on the CPU, or on the device where the host einsum would take over a second"""
    C, B, Do, L = ops.u.shape
    return DEV if C * B * Do * ops.v.shape[1] * L > 2e7 else "cpu"


def guarded(*shape):
    """a zeroed output in the middle of a -0.0-filled buffer: -0.0 + 0.0 = +0.0 flips the sign bit of whatever a kernel
    read-modify-writes outside its output (tests/test_gpu_kernels.py::test_gram_direct_epilogue_stays_inside_the_matrix)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((2 * PAD + n,), -0.0, device=DEV)
    out = buf[PAD:PAD + n].view(*shape)
    out.zero_()
    return buf, out


def untouched(buf, n):
    return bool(torch.signbit(buf[:PAD]).all() and torch.signbit(buf[PAD + n:]).all())


def misaligned(t):
    """a contiguous copy of ``t`` four bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def aligned16(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


# ---- the planes form ---------------------------------------------------------------------------------------------------------
@params("planes")
def test_planes_instance(row):
    """L swept over Q = 1 ... 8 chunks per workgroup (both sides of every ring depth), B = 3 and 8 (the XCD remap on at 8),
    v with one scale per sample and with one for the tensor, both spectra; nothing is written outside fvar [B, C, C]
    (padded outputs c >= C are staged as zeros and dropped by the reduction); a second call doubles the result.  The
    ``stream`` rows walk several tiles per workgroup with several chunks per tile."""
    k = K()
    C, Do, Dk = row["C"], row["Do"], row["Dk"]
    for B in row["Bs"]:
        full = qf.to_device(qf.operands(C, B, Do, Dk, max(row["Ls"]), qf.row_seed(row) + B), DEV)
        for L in row["Ls"]:
            var = k.quadform_shared_variant(qf.QF_PLANES, B, C, Do, Dk, L)
            want_var = dict(qf.planes_expectation(row), ct=qf.class_tile(C))
            assert {x: var[x] for x in want_var} == want_var, (var, want_var)
            if row.get("stream"):
                assert var["split"] < qf.ntiles(Do, Dk) and L > 16
            ops = qf.first_positions(full, L)
            ref_dev = reference_device(ops)
            for spectrum in qf.SPECTRA:
                o = qf.with_spectrum(ops, spectrum)
                r = qf.to_device(o, ref_dev)
                want = qf.reference_fvar(r.u, r.v, qf.kron_weights(r.l1, r.l2, r.delta))
                for per_image in (True, False):
                    what = f"B{B} L{L} {spectrum} {'per-image' if per_image else 'one-scale'}"
                    buf, fvar = guarded(B, C, C)
                    qf.run_planes(k, o, per_image, fvar)
                    assert untouched(buf, B * C * C), f"{what}: wrote outside fvar"
                    held(fvar, want, 2, what)
                qf.run_planes(k, o, False, fvar)
                assert untouched(buf, B * C * C), "second call wrote outside fvar"
                held(fvar, 2 * want, 2, f"B{B} L{L} {spectrum} accumulated")


# ---- fp32 operands -----------------------------------------------------------------------------------------------------------
def _fp32_weights(o, route):
    return o.var_w.double() if route == "diag" else qf.kron_weights(o.l1, o.l2, o.delta)


@params("fp32")
def test_fp32_instance(row):
    """Kronecker (sample- and seed-major u) and diagonal weights; ARITH 1 on whole float4s, ARITH 0 at L % 4 != 0 and behind
    a 4-byte offset of u; the ``multitile`` rows walk several tiles per workgroup (the next-tile prefetch).  Against fp64, and
    route against route: the other layout of u, and the other weight form on the same weights."""
    k = K()
    C, Do, Dk, route = row["C"], row["Do"], row["Dk"], row["route"]
    shapes = [(B, L, False) for B in row["Bs"] for L in row["Ls"]] + [(B, L, True) for B in row["Bs"] for L in row.get("offset_Ls", ())]
    for B, L, offset in shapes:
        ops = qf.to_device(qf.operands(C, B, Do, Dk, L, qf.row_seed(row) + L), DEV)
        u = ops.u if route == "kron-seedmajor" else qf.sample_major(ops.u)
        if offset:
            u = misaligned(u)
        var = k.quadform_shared_variant(qf.row_form(row), B, C, Do, Dk, L, aligned16(u, ops.v))
        assert (var["ct"], var["arith"]) == (qf.class_tile(C), row["arith"]), var
        if row.get("multitile"):
            assert var["split"] < qf.ntiles(Do, Dk)
        ref_dev = reference_device(ops)
        for spectrum in qf.SPECTRA:
            o = qf.with_spectrum(ops, spectrum)
            r = qf.to_device(o, ref_dev)
            want = qf.reference_fvar(r.u, r.v, _fp32_weights(r, route))
            what = f"B{B} L{L}{' offset' if offset else ''} {spectrum}"
            buf, fvar = guarded(B, C, C)
            qf.run_fp32(k, o, route, fvar, u=u)
            assert untouched(buf, B * C * C), f"{what}: wrote outside fvar"
            held(fvar, want, 2, what)
            assert torch.equal(qf.run_fp32(k, o, route, u=u), fvar), f"{what}: not reproducible"  # fixed-order reduction
            # the other layout of u (the same kernel behind other strides), and Kronecker against diagonal weights
            other = {"kron": "kron-seedmajor", "kron-seedmajor": "kron", "diag": "kron"}[route]
            routes_agree(qf.run_fp32(k, o, other), fvar, 1, 1e-5 if "diag" in (route, other) else 4e-6, f"{what} vs {other}")
            qf.run_fp32(k, o, route, fvar, u=u)
            held(fvar, 2 * want, 2, what + " accumulated")


# ---- the exact GGN diagonal --------------------------------------------------------------------------------------------------
@params("diag_ggn")
def test_diag_ggn_instance(row):
    """S = 1 ... 10 seeds on both tile products; the ``manysamples`` rows give a workgroup more than one sample (the
    `n += nsplit` walk and its prefetch of the next sample).  Bit-reproducible; accumulates with alpha."""
    k = K()
    S, Do, Dk = row["C"], row["Do"], row["Dk"]
    for B in row["Bs"]:
        for L in row["Ls"]:
            ops = qf.to_device(qf.operands(S, B, Do, Dk, L, qf.row_seed(row) + L), DEV)
            var = k.quadform_shared_variant(qf.QF_DIAG_GGN, B, S, Do, Dk, L, aligned16(ops.u, ops.v))
            assert (var["ct"], var["arith"]) == (qf.class_tile(S), row["arith"]), var
            if row.get("manysamples"):
                assert var["split"] < B
            r = qf.to_device(ops, reference_device(ops))
            want = qf.reference_diag_ggn(r.u, r.v)
            buf, h = guarded(Do * Dk)
            qf.run_diag_ggn(k, ops, 1.0, h)
            assert untouched(buf, Do * Dk), "wrote outside h"
            held(h, want, 1, f"B{B} L{L}")
            assert torch.equal(qf.run_diag_ggn(k, ops, 1.0), h)
            qf.run_diag_ggn(k, ops, 0.5, h)
            held(h, 1.5 * want, 1, f"B{B} L{L} accumulated")


# ---- the prior-precision grid ------------------------------------------------------------------------------------------------
@params("grid")
def test_shared_grid_instance(row):
    """CT = 5 (3, 4, 5 outputs) and a short second block inside CT = 10 next to the counts the older test has, three weight
    modes, both tile products, both layouts of u; one row walks several tiles per workgroup.  Against fp64, and for the
    Kron and diagonal modes against G calls of the single-delta kernels."""
    k = K()
    C, Do, Dk, mode, seed_major = row["C"], row["Do"], row["Dk"], row["mode"], row["seed_major"]
    deltas = qf.DELTAS.to(DEV)
    for B in row["Bs"]:
        for L in row["Ls"]:
            ops = qf.to_device(qf.operands(C, B, Do, Dk, L, qf.row_seed(row) + L), DEV)
            var = k.quadform_shared_variant(qf.QF_GRID, B, C, Do, Dk, L, aligned16(ops.u, ops.v))
            assert (var["ct"], var["arith"]) == (qf.class_tile(min(C, 10), qf.GRID_CLASS_TILES), row["arith"]), var
            if row.get("multitile"):
                assert var["split"] < qf.ntiles(Do, Dk)
            ref_dev = reference_device(ops)
            for spectrum in qf.SPECTRA:
                o = qf.with_spectrum(ops, spectrum)
                r = qf.to_device(o, ref_dev)
                want = qf.reference_grid_var(r.u, r.v, qf.grid_weights(mode, r.l1, r.l2, qf.DELTAS.to(ref_dev)))
                got = qf.run_grid(k, o, mode, seed_major, deltas)
                held(got, want, 1, f"B{B} L{L} {spectrum}")
                assert torch.equal(qf.run_grid(k, o, mode, seed_major, deltas), got)
                if C <= 10 and mode != 1:
                    single = torch.empty_like(got)
                    for g, d in enumerate(deltas):
                        if mode == 0:
                            od = SimpleNamespace(**{**vars(o), "delta": d.reshape(1)})
                            fv = qf.run_fp32(k, od, "kron-seedmajor" if seed_major else "kron")
                        else:
                            od = SimpleNamespace(**{**vars(o), "var_w": (1.0 / (qf.grid_diag_h(o.l1, o.l2) + d)).contiguous()})
                            fv = qf.run_fp32(k, od, "diag")
                        single[g] = torch.diagonal(fv, dim1=1, dim2=2)
                    routes_agree(got, single, 2, 1e-5, f"B{B} L{L} {spectrum} vs single-delta kernels")


@params("linear_grid")
def test_linear_grid_instance(row):
    """the nn.Linear grid kernel where the grid points are walked in LDS pieces (GS = 4 < G = 9) and where the staged
    activations alone exceed 64 KiB (the raised dynamic-LDS limit, GS = 1); three modes, with and without the bias block"""
    k = K()
    C, Do, Di, mode, bias = row["C"], row["Do"], row["Dk"], row["mode"], row["bias"]
    deltas = qf.DELTAS.to(DEV)
    for B in row["Bs"]:
        for spectrum in qf.SPECTRA:
            o = qf.to_device(qf.linear_operands(C, B, Do, Di, qf.row_seed(row), spectrum), DEV)
            W = qf.grid_weights(mode, o.l1, o.l2, deltas)
            want = qf.reference_linear_grid_var(o.u, o.v, W, *((o.ub, o.wb, deltas) if bias else ()))
            got = qf.run_linear_grid(k, o, mode, bias, deltas)
            held(got, want, 1, f"B{B} {spectrum}")
            assert torch.equal(qf.run_linear_grid(k, o, mode, bias, deltas), got)
