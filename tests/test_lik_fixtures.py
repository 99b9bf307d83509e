"""The likelihood fixtures (tests/lik_fixtures.py) are well-posed for fp32: a careful float32 evaluation of the kernels'
closed forms -- the row maximum subtracted first -- meets, on every case and every metric, the bound that
tests/test_gpu_lik.py asks of the device, so a failure there is the kernel's, not the input's.  And the cases discriminate:
the order ``logz = log z + m``, ``p_j = exp(f_j - logz)`` (what csrc/lk_lik.hip computed before the roots took the shift
first) misses the same bound on the batches shifted by 1000."""
import pytest
import torch

from tests import lik_fixtures as LF
from tests.lik_fixtures import BOUND

CASES = {False: LF.cases(False), True: LF.cases(True)}
ROOTS = [(ch, c) for ch in (False, True) for c in CASES[ch]]
_ids = [f"{'chol' if ch else 'sym'}-{c.name}" for ch, c in ROOTS]


def kernel_order_f32(case, cholesky, base=LF.LOSS_BASE):
    """the same closed forms with the maximum added back into the log-partition before it is subtracted: logz carries
    an error of an ulp of |m|, which p and the loss inherit"""
    f = case.f.float()
    m = f.max(1, keepdim=True).values
    e = torch.exp(f - m)
    z = e.sum(1, keepdim=True)
    logz = torch.log(z) + m
    p = torch.exp(f - logz)
    rows, am = torch.arange(f.shape[0]), f.argmax(1)
    rest = e.clone()
    rest[rows, am] = 0.0
    top = (am, p[rows, am].sqrt() * (rest.sum(1) / z.squeeze(1)))  # (as the careful evaluation: only the order of logz differs)
    valid = case.y >= 0
    fl = f.gather(1, case.y.clamp(min=0).view(-1, 1))
    nll = torch.where(valid, (logz - fl).squeeze(1), torch.zeros(f.shape[0]))
    return LF.roots_from_p(p, cholesky, top=top), (torch.tensor(base, dtype=torch.float32) + nll.sum()).item()


@pytest.mark.parametrize("cholesky,case", ROOTS, ids=_ids)
def test_careful_fp32_meets_the_bound(cholesky, case):
    S, after = LF.careful_f32(case, cholesky)
    B, C = case.f.shape
    assert LF.structure_ok(S, C, cholesky)
    root, lam, loss = LF.errors(case, cholesky, S, after)
    print(f"{case.name}: root {root:.2e} S S^T {lam:.2e} loss {loss if loss is None else format(loss, '.2e')}")
    assert root < BOUND and lam < BOUND, (case.name, root, lam)
    if loss is None:
        assert after == LF.LOSS_BASE, "no valid label: nothing is added"
    else:
        assert loss < BOUND, (case.name, loss)


@pytest.mark.parametrize("cholesky,case", ROOTS, ids=_ids)
def test_no_expected_entry_is_decided_by_denormals(cholesky, case):
    """every non-zero entry of the expected root is above 1e-30 in magnitude, and so is the largest entry of every sample's
    Lambda that is not all zero (the figure S S^T is normalised by)"""
    S, Lam, loss = LF.reference(case, cholesky)
    nz = S[S != 0].abs()
    assert nz.numel() == 0 or nz.min().item() > 1e-30, nz.min().item()
    top = Lam.abs().reshape(Lam.shape[0], -1).amax(1)
    assert bool(((top == 0) | (top > 1e-30)).all())
    assert loss >= 0 and (loss == 0 or loss > 1e-30)
    assert torch.equal(case.f, case.f.float().double()), "the logits are fp32 numbers"
    assert bool(torch.isfinite(case.f).any(1).all()), "no row is masked entirely"
    valid = case.y >= 0
    lab = case.f.gather(1, case.y.clamp(min=0).view(-1, 1)).squeeze(1)
    assert bool(torch.isfinite(lab[valid]).all()), "no label is masked"


def test_kernel_order_misses_the_bound_at_shift_1000():
    """the cases discriminate: with logz = log z + m every mixed batch shifted by 1000 is off by more than the bound on
    the root (and the large ones on the loss), while no unshifted batch is"""
    seen = 0
    for cholesky in (False, True):
        for case in CASES[cholesky]:
            if not case.name.startswith("mixed") or "ignall" in case.name:
                continue
            root, lam, loss = LF.errors(case, cholesky, *kernel_order_f32(case, cholesky))
            if "shift1000" in case.name:
                seen += 1
                print(f"{case.name}: root {root:.2e} S S^T {lam:.2e} loss {loss:.2e}")
                assert root > BOUND or lam > BOUND or loss > BOUND, (case.name, root, lam, loss)
            elif "shift0" in case.name:
                assert root < BOUND and lam < BOUND and loss < BOUND, (case.name, root, lam, loss)
    assert seen >= 2 * 14


def test_the_cases_are_what_they_say():
    for cholesky in (False, True):
        names = [c.name for c in CASES[cholesky]]
        assert len(set(names)) == len(names)
        shapes = {tuple(c.f.shape) for c in CASES[cholesky]}
        assert {(B, C) for B in LF.BATCHES for C in LF.CLASSES} <= shapes
        assert ((5, 1000) in shapes) == cholesky
        assert any(set(c.families) == set(LF.FAMILIES) for c in CASES[cholesky]), "a batch with rows of every family"
        assert any(bool((c.y == LF.IGNORE).all()) for c in CASES[cholesky])
        assert any(bool((c.y == LF.IGNORE).any()) and not bool((c.y == LF.IGNORE).all()) for c in CASES[cholesky])
    a, b = LF.batch(130, 10, 1000), LF.batch(130, 10, 1000)
    assert torch.equal(a.f, b.f) and torch.equal(a.y, b.y), "seeded: the same batch every time"
    f0 = LF.batch(130, 10, 0).f
    fin = torch.isfinite(f0)
    assert bool(((a.f - f0)[fin] - 1000).abs().max() < 1e-4), "the shifted batch is the same batch"
    p = torch.softmax(a.f, 1)
    for r, fm in enumerate(a.families[:len(LF.FAMILIES)]):
        if fm.startswith("correct"):
            assert p[r, a.y[r] if a.y[r] >= 0 else p[r].argmax()] > 1 - 10 * 2.72 ** -int(fm[7:])
        if fm in ("first", "middle", "last"):
            assert int(p[r].argmax()) == {"first": 0, "middle": 5, "last": 9}[fm]
        if fm == "tie_all":
            assert bool((p[r] == 0.1).all())
        if fm == "masked1":
            assert int((p[r] == 0).sum()) == 1
        if fm == "maskedN":
            assert int((p[r] == 0).sum()) == 5


def test_metrics_see_a_wrong_row():
    """the per-sample figures are ~0 for the fp64 reference itself and react to damage in a saturated row that the
    whole-tensor norm of tests/test_gpu_kernels.py does not see"""
    case = LF.batch(130, 10, 0)
    for cholesky in (False, True):
        S, Lam, loss = LF.reference(case, cholesky)
        assert LF.row_err(S, S) == 0 and LF.lam_err(S, Lam) < 1e-12
        r = case.families.index("correct30")
        bad = S.clone()
        bad[:, r, :] *= 1 + 1e-3
        assert LF.row_err(bad, S) > 9e-4 and LF.lam_err(bad, Lam) > 1e-3
        assert (bad - S).abs().max().item() / S.abs().max().item() < 1e-8, "invisible to one global norm"
        z = torch.zeros(3, 2, 4)
        assert LF.row_err(z, z) == 0
        z2 = z.clone()
        z2[1, 0, 2] = 1e-40
        assert LF.row_err(z2, z) == float("inf"), "an all-zero sample must come back as exact zeros"
        z2[0, 1, 0] = float("nan")
        assert LF.row_err(z2, z) != LF.row_err(z2, z)
    S = LF.reference(case, True)[0]
    assert LF.structure_ok(S, 10, True)
    S[4, 7, 2] = 1e-30
    assert not LF.structure_ok(S, 10, True)
    assert LF.loss_err(1.0 + 1e-3, 1.0) == pytest.approx(1e-3)


@pytest.mark.parametrize("kind", LF.SQ_KINDS)
@pytest.mark.parametrize("numel", LF.SQ_NUMELS)
def test_sq_err_careful_fp32_meets_the_bound(numel, kind):
    f, y = LF.sq_case(numel, kind)
    assert torch.equal(f, f.float().double()) and torch.equal(y, y.float().double())
    want, got = LF.sq_reference(f, y), LF.sq_careful_f32(f, y)
    if kind == "equal":
        assert want == 0 and got == LF.LOSS_BASE
    else:
        e = LF.loss_err(got, LF.LOSS_BASE + want)
        print(f"sq_err numel={numel} {kind}: {e:.2e}")
        assert want > 0 and e < BOUND
