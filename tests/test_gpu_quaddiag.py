"""The diagonal-output predictive kernels (csrc/lk_quaddiag.hip) on the MI355X against the fp64 definition

    fvar_diag[n][c] = sum_{o,i} (sum_l u[n,c,o,l] v[n,i,l])^2 w[o,i]

held to |got - want| <= 1e-4 |want| + 1e-6 max|want| per sample (tests/quad_fixtures.py), on the operands of the full form's
tests: correlated, differently scaled outputs, post-ReLU inputs over five decades, a flat and a clamped KFAC spectrum.  A case is
named by the path ``lk_quaddiag_variant`` reports for it and asks the query that it takes that path.  Every launch accumulates
into a prefilled output between guard bands, over a NaN-filled workspace, twice with equal bits.  End to end:
``diagonal_output=True`` of the Kron and diagonal Laplace against diag(J Sigma J^T) in fp64.  Measured ratios:
profiles/quaddiag_instances.md."""
import copy
import math

import pytest
import torch
from torch import nn

from tests import quad_fixtures as qf
from tests.parity_log import record_error

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 1024
RESIDENT_MAX_L = 64  # QD_RESIDENT_MAX_L


def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


def held(got, want, what):
    ratio = record_error(qf.tolerance_ratio(got, want, 1))
    print(f"{what}: |err| / tolerance = {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: |err| / tolerance = {ratio:.3g}"


def accumulated_twice(launch, want, what, k, ws_bytes=0):
    """``launch(out)`` adds into a prefilled [B, C] between -0.0 guard bands (a stray read-modify-write flips their sign bit),
    over a NaN workspace; two runs give the same bits; what was added is held to the bound"""
    B, C = want.shape
    pre = ((torch.arange(B * C, device=DEV) % 7 + 1).float().view(B, C) * 0.125 * want.float().to(DEV))
    outs = []
    for _ in range(2):
        buf = torch.full((2 * PAD + B * C,), -0.0, device=DEV)
        out = buf[PAD:PAD + B * C].view(B, C)
        out.copy_(pre)
        if ws_bytes:
            k._workspace(ws_bytes, torch.device(DEV, torch.cuda.current_device())).fill_(255)  # every float a NaN
        launch(out)
        assert bool(torch.signbit(buf[:PAD]).all() and torch.signbit(buf[PAD + B * C:]).all()), f"{what}: wrote outside"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), f"{what}: two runs differ"
    held(outs[0].double() - pre.double(), want, what)


# (C, Do, Dk, L, form, spectrum, seed_major, B): thinned to the distinct paths — arithmetic (L % 4), resident / streamed v
# (L <= 64), one chunk short / full (C = 1, 7, 8), a moved-back last chunk (9, 17, 100), partial / exact / several super-tiles,
# and at B = 264 several super-tiles per workgroup on the XCD-aware mapping
PAST = RESIDENT_MAX_L + 4
SHARED = [(C, 33, 130, 16, "kron", "flat", False, 3) for C in (1, 7, 8, 9, 17, 100)]
SHARED += [(C, 33, 130, 3, "diag", "kfac", True, 3) for C in (1, 7, 8, 9, 17, 100)]
SHARED += [(C, 33, 130, L, f, s, sm, 3) for C in (9, 100) for L in (PAST, PAST - 1)
           for f, s, sm in (("kron", "kfac", True), ("diag", "flat", False))]
SHARED += [(17, Do, Dk, L, f, "kfac", sm, 3) for Do, Dk in ((5, 27), (32, 128))
           for L, f, sm in ((3, "kron", False), (16, "diag", True), (PAST, "kron", True))]
SHARED += [(9, 64, 640, L, "kron", "flat", sm, 264) for L, sm in ((3, True), (16, False), (PAST, False))]


def shared_path(C, L):
    return dict(arith=int(L % 4 == 0), resident=L <= RESIDENT_MAX_L, chunks=-(-C // 8), rem=C % 8)


def shared_id(case):
    C, Do, Dk, L, form, spectrum, sm, B = case
    p = shared_path(C, L)
    return (f"{form}-{spectrum}-{'seedmajor' if sm else 'batchmajor'}-arith{p['arith']}-{'resident' if p['resident'] else 'streamed'}"
            f"-chunks{p['chunks']}rem{p['rem']}-C{C}-Do{Do}-Dk{Dk}-L{L}-B{B}")


@pytest.mark.parametrize("case", SHARED, ids=[shared_id(c) for c in SHARED])
def test_shared_kernel(case):
    C, Do, Dk, L, form, spectrum, seed_major, B = case
    k = K()
    var = k.quaddiag_variant(k.QD_KRON if form == "kron" else k.QD_DIAG, B, C, Do, Dk, L)
    assert {x: var[x] for x in ("arith", "resident", "chunks", "rem")} == shared_path(C, L), var
    if B > 3:
        assert var["split"] < qf.ntiles(Do, Dk) and (B * var["split"]) % (8 * var["split"]) == 0
    ops = qf.to_device(qf.operands(C, B, Do, Dk, L, 1000 * C + L + B, spectrum), DEV)
    w = qf.kron_weights(ops.l1, ops.l2, ops.delta) if form == "kron" else ops.var_w.double()
    r = ops if B > 3 else qf.to_device(ops, "cpu")  # (the large case's fp64 einsum runs on the device)
    want = qf.reference_grid_var(r.u, r.v, w.to(r.u.device)[None])[0]
    u = ops.u if seed_major else qf.sample_major(ops.u)
    assert u.data_ptr() % 16 == 0 and ops.v.data_ptr() % 16 == 0
    if form == "kron":
        launch = lambda out: k.kron_quaddiag_shared(u, ops.v, ops.l1, ops.l2, ops.delta, out, seed_major=seed_major)
    else:
        launch = lambda out: k.diag_quaddiag_shared(u, ops.v, ops.var_w, out, seed_major=seed_major)
    accumulated_twice(launch, want, shared_id(case), k, k.lib.lk_quaddiag_shared_workspace_bytes(B, C, Do, Dk))


@pytest.mark.parametrize("Di", [3, 128])
@pytest.mark.parametrize("Do", [5, 64, 65])
@pytest.mark.parametrize("C", [1, 11, 100])
def test_linear_kernels(C, Do, Di):
    k, B = K(), 3
    for spectrum, bias in (("flat", False), ("kfac", True)):
        ops = qf.to_device(qf.linear_operands(C, B, Do, Di, 7 * C + Do + Di, spectrum), DEV)
        u2, v2, ub2 = ops.u.double().cpu() ** 2, ops.v.double().cpu() ** 2, ops.ub.double().cpu() ** 2
        delta_b = torch.tensor([0.3], device=DEV)
        wbias = 1.0 / (ops.wb.double().cpu() + 0.3)
        want = torch.einsum("cno,ni,oi->nc", u2, v2, qf.kron_weights(ops.l1, ops.l2, ops.delta).cpu())
        if bias:
            want = want + torch.einsum("cno,o->nc", ub2, 1.0 / (ops.wb.double().cpu() + delta_b.double().cpu()))
        accumulated_twice(lambda out: k.kron_quaddiag_linear(ops.u, ops.v, ops.l1, ops.l2, ops.delta, out, *(
            (ops.ub, ops.wb, delta_b) if bias else ())), want, f"kron {spectrum} bias={bias}", k)
        var_b = wbias.float().to(DEV)
        want = torch.einsum("cno,ni,oi->nc", u2, v2, ops.var_w.double().cpu())
        if bias:  # (the diagonal posterior's bias block reads the gradients themselves)
            want = want + torch.einsum("cno,o->nc", u2, var_b.double().cpu())
        accumulated_twice(lambda out: k.diag_quaddiag_linear(ops.v, ops.u, ops.var_w, var_b if bias else None, out), want,
                          f"diag {spectrum} bias={bias}", k)


def test_argument_checks():
    from laplace_amd._lib import LaplaceHipError

    k = K()
    ops = qf.to_device(qf.operands(2, 3, 5, 27, 4, 1), DEV)
    u, out = qf.sample_major(ops.u), torch.zeros(3, 2, device=DEV)
    need = k.lib.lk_quaddiag_shared_workspace_bytes(3, 2, 5, 27)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    args = (u.data_ptr(), ops.v.data_ptr(), ops.l1.data_ptr(), ops.l2.data_ptr(), ops.delta.data_ptr())
    assert need == 3 * 1 * 2 * 4 and k.lib.lk_quaddiag_shared_workspace_bytes(3, 4097, 5, 27) == 0
    assert k.lib.lk_kron_quaddiag_shared_f32(*args, 3, 2, 5, 27, 4, 0, out.data_ptr(), ws.data_ptr(), need - 1, None) == -1
    assert k.lib.lk_kron_quaddiag_shared_f32(*args, 3, 4097, 5, 27, 4, 0, out.data_ptr(), ws.data_ptr(), need, None) == -1
    assert k.lib.lk_diag_quaddiag_shared_f32(*args[:3], 3, 4097, 5, 27, 4, 0, out.data_ptr(), ws.data_ptr(), need, None) == -1
    assert k.lib.lk_kron_quaddiag_linear_f32(*args, 3, 4097, 5, 27, None, None, None, out.data_ptr(), None) == -1
    assert k.quaddiag_variant(k.QD_KRON, 3, 4097, 5, 27, 4) is None and k.QUADDIAG_MAX_C == 4096
    torch.cuda.synchronize()
    assert not out.any()
    with pytest.raises(LaplaceHipError):
        k.kron_quaddiag_shared(u, ops.v, ops.l1, ops.l2, ops.delta, torch.zeros(3, 3, device=DEV))


# ---- end to end ------------------------------------------------------------------------------------------------------------
class ConvNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1, self.c2, self.fc = nn.Conv2d(3, 6, 3, padding=1), nn.Conv2d(6, 8, 3, stride=2, padding=1), nn.Linear(128, 12)

    def forward(self, x):
        return self.fc(torch.flatten(torch.relu(self.c2(torch.relu(self.c1(x)))), 1))


class SeqNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(5, 16), nn.Linear(16, 12)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x))).mean(1)


class Loader(list):
    dataset = list(range(16))


def reference_variance(la, model, X):
    """diag(J Sigma J^T) [B, C] in fp64: torch.func.jacrev Jacobians of the fp64 model against the posterior the device holds"""
    m64 = copy.deepcopy(model).double().cpu()
    params = {n: p.detach() for n, p in m64.named_parameters()}
    jac = torch.func.jacrev(lambda p: torch.func.functional_call(m64, p, (X.double().cpu(),)))(params)
    Js = [jac[n].flatten(2) for n in params]  # [B, C, numel] per parameter, in parameter order
    if la._structure == "diag":
        return torch.einsum("ncp,p->nc", torch.cat(Js, 2) ** 2, la.posterior_variance.double().cpu())
    post, var = la.posterior_precision, 0.0
    for J, Qs, ls, delta in zip(Js, post.eigenvectors, post.eigenvalues, post.deltas):
        Qs, ls, delta = [Q.double().cpu() for Q in Qs], [l.double().cpu() for l in ls], delta.double().cpu()
        if len(ls) == 1:
            var = var + ((J @ Qs[0]) ** 2 / (ls[0] + delta)).sum(-1)
        else:
            R = torch.einsum("op,ncoi,iq->ncpq", Qs[0], J.reshape(*J.shape[:2], len(ls[0]), len(ls[1])), Qs[1])
            var = var + (R ** 2 / (torch.outer(ls[0], ls[1]) + delta)).sum((-1, -2))
    return var


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("net", [ConvNet, SeqNet])
def test_diagonal_output_end_to_end(net, structure, monkeypatch):
    from laplace_amd import predictive as P
    from laplace_amd.laplace import HipLaplace

    torch.manual_seed(11)
    model = net().to(DEV)
    X = torch.randn(16, 3, 8, 8, device=DEV) if net is ConvNet else torch.randn(16, 6, 5, device=DEV)
    y = torch.randint(12, (16,), device=DEV)
    la = HipLaplace(model, "classification", "all", structure, prior_precision=0.7)
    la.fit(Loader([(X[:8], y[:8]), (X[8:], y[8:])]))
    assert P.use_diag_output_kernels and P.diag_output_min_outputs == 11  # 12 outputs: the new route is the default one
    f_mu, var_on = la._glm_predictive_distribution(X[:4], diagonal_output=True)
    assert var_on.shape == (4, 12)
    held(var_on, reference_variance(la, model, X[:4]), "diagonal-output kernels")
    monkeypatch.setattr(P, "use_diag_output_kernels", False)
    var_off = la._glm_predictive_distribution(X[:4], diagonal_output=True)[1]
    assert var_off.shape == (4, 12)
    held(var_off, var_on.double(), "[B, C, C] route against the diagonal-output kernels")
    monkeypatch.undo()
    probit = torch.softmax(f_mu.double() / torch.sqrt(1.0 + math.pi / 8 * var_on.double()), -1)
    held(la(X[:4], diagonal_output=True), probit, "probit link on the diagonal")
