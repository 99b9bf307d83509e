"""Shapes, inputs and references for the slicing kernels (csrc/lk_slice.hip) and the small CSP / class-token networks of the
end-to-end tests - shared by tests/test_slice_fixtures.py (CPU: the table reaches every path, the references bite),
tests/emulated_slice_kernels.py (the kernel emulation states its rule through `vjp_reference`), tests/test_sweep_slice.py and
tests/test_gpu_slice.py (the device).

A kernel case is a dict: rows ``R``, row length ``Ct``, ``pieces`` (per piece ``(c0, cs, kind)`` with kind ``"f32"`` or
``"split"``, in the listed order), ``sexp`` (per split piece), ``off`` (1: every buffer starts one element past an aligned
address), ``cancel`` (the pieces hold the values of a cancellation row: another order of the sum changes the result) and ``wide``
(the lane index passes 2^31: checked by shape only, never run).  The shapes are the smallest at which a path can go wrong: one
row and three, rows of 5, 8 and 12 columns, pieces at columns 0, 1 and 4, one and eight pieces, every mix of fp32 and split pieces
in a row of three, columns no piece covers, pieces that overlap or repeat, unaligned bases, more than one workgroup, one lane
past a full stride of the grid (2048 workgroups of 256 lanes) on the vector and on the scalar path, and no rows at all.
"""
import itertools

import torch
from torch import nn

GRID_LANES = 2048 * 256  # lanes of one stride of the grid (SLICE_MAX_BLOCKS x 256 of csrc/lk_slice.hip)
MAX_PIECES = 8
FILL = 7.0  # what the mutant that drops the zero fill finds in memory


def _case(R, Ct, pieces, sexp=(3, -2, 0, 7, 1, -1, 2, 4), off=0, cancel=False, wide=False):
    pieces = tuple((c0, cs, kind) for c0, cs, kind in pieces)
    n_split = sum(k == "split" for _, _, k in pieces)
    return dict(R=R, Ct=Ct, pieces=pieces, sexp=tuple(sexp[:n_split]), off=off, cancel=cancel, wide=wide)


_MIX3 = list(itertools.product(("f32", "split"), repeat=3))  # every mix of fp32 and split pieces in a row of three

CASES = [
    # the smallest shapes: R in {1, 3}, Ct in {5, 8, 12}, c0 in {0, 1, 4}; one piece, with columns no piece covers
    *[_case(R, Ct, [(c0, cs, kind)], off=off)
      for (R, Ct, c0, cs, kind, off) in [(1, 5, 0, 5, "f32", 0), (1, 5, 1, 3, "split", 0), (3, 5, 4, 1, "f32", 1), (1, 8, 0, 4, "split", 0),
                                         (3, 8, 4, 4, "f32", 0), (3, 8, 1, 4, "f32", 0), (1, 12, 4, 8, "split", 0), (3, 12, 4, 4, "f32", 0),
                                         (3, 12, 0, 12, "split", 1), (3, 12, 1, 7, "split", 0), (1, 12, 0, 4, "f32", 0)]],
    # every mix of three pieces: a chunk into three on the vector path (Ct = 12), and overlapping ranges on the scalar path
    *[_case(3, 12, [(0, 4, a), (4, 4, b), (8, 4, c)]) for a, b, c in _MIX3],
    *[_case(3, 5, [(0, 3, a), (1, 4, b), (1, 1, c)], off=i % 2) for i, (a, b, c) in enumerate(_MIX3)],
    # a full-width part with two slices of it, one of them twice (overlap and repetition), and columns [8, 12) under the full part alone
    _case(3, 12, [(0, 12, "split"), (0, 4, "f32"), (4, 4, "split"), (4, 4, "split")]),
    # eight pieces: the halves of a chunk with full-width parts (vector), and a ragged ladder with a hole at column 0 (scalar)
    _case(3, 8, [(0, 8, "f32"), (0, 4, "split"), (4, 4, "f32"), (0, 8, "split"), (4, 4, "split"), (0, 4, "f32"), (0, 8, "f32"), (4, 4, "split")]),
    _case(3, 12, [(1, 2, "f32"), (2, 3, "split"), (4, 1, "f32"), (4, 8, "split"), (5, 5, "f32"), (11, 1, "split"), (1, 11, "f32"), (3, 3, "split")]),
    # the cancellation row: 2^25, -2^25 and 1 over the same columns - only the listed order gives 1
    _case(3, 8, [(0, 8, "f32"), (0, 8, "f32"), (0, 8, "f32")], cancel=True),
    _case(1, 5, [(0, 5, "f32"), (1, 4, "split"), (1, 4, "f32")], cancel=True),
    # an unaligned base with a shape that would otherwise take 16-byte accesses
    _case(3, 8, [(0, 4, "f32"), (4, 4, "split")], off=1),
    # more than one workgroup; one short of / at / one past a wave of lanes
    _case(257, 12, [(0, 4, "f32"), (4, 8, "split"), (0, 12, "f32")]), _case(63, 5, [(1, 3, "split")]),
    _case(64, 4, [(0, 4, "f32")]), _case(65, 4, [(0, 4, "split")]), _case(13, 5, [(0, 2, "f32"), (4, 1, "split")]),
    # one lane past a full stride of the grid: one lane per row on the vector path (Ct = 4), and on the scalar path (Ct = 5)
    _case(GRID_LANES + 1, 4, [(0, 4, "f32"), (0, 4, "split")]),
    _case(GRID_LANES // 5 + 1, 5, [(1, 3, "split"), (0, 5, "f32"), (4, 1, "f32")]),
    # no rows
    _case(0, 8, [(0, 4, "f32"), (4, 4, "split")]),
    # the lane index passes 2^31 (by shape only): 2^31 + 1 rows of one lane would be 32 GiB
    _case((1 << 31) + 1, 1, [(0, 1, "f32")], wide=True), _case((1 << 31) + 4, 4, [(0, 4, "f32")], wide=True),
]


def case_id(c):
    return (f"R{c['R']}-Ct{c['Ct']}-" + ".".join(f"{c0}+{cs}{'s' if k == 'split' else 'f'}" for c0, cs, k in c["pieces"])
            + ("-unaligned" if c["off"] else "") + ("-cancel" if c["cancel"] else "") + ("-wide" if c["wide"] else ""))


def split_mask(c):
    return sum(1 << i for i, (_, _, k) in enumerate(c["pieces"]) if k == "split")


def make_pieces(c, gen):
    """the pieces of a case on the CPU: per piece ``(value, c0, cs)`` with ``value`` an fp32 ``[R, cs]`` tensor, or ``(hi, lo, sexp)``
    - fp16 planes ``[R, cs]`` and an int - whose value is ``(float(hi) + float(lo)) * 2^-sexp``.  Finite, no integers; the scales
    keep every value far from the subnormals.  A cancellation case holds 2^25, -2^25 and 1 in its first three pieces (a split
    piece: +-2^10 in ``hi`` at ``sexp = -15``, or 1 at ``sexp = 0``, with ``lo`` zero - halves times a power of two)."""
    out, k = [], 0
    for i, (c0, cs, kind) in enumerate(c["pieces"]):
        if c["cancel"]:
            big = (2.0 ** 25, -2.0 ** 25, 1.0)[i]
            if kind == "f32":
                out.append((torch.full((c["R"], cs), big), c0, cs))
            else:  # (2^25 is no half: 2^10 at the scale 2^15, i.e. sexp = -15)
                mant, sexp = (2.0 ** 10, -15) if abs(big) > 1 else (1.0, 0)
                out.append(((torch.full((c["R"], cs), mant if big > 0 else -mant).half(), torch.zeros(c["R"], cs).half(), sexp), c0, cs))
                k += 1
        elif kind == "f32":
            out.append((torch.randn(c["R"], cs, generator=gen) * 1.7 + 0.01, c0, cs))
        else:
            hi = torch.randn(c["R"], cs, generator=gen).half()
            lo = (torch.randn(c["R"], cs, generator=gen) * 2.0 ** -11).half()
            out.append(((hi, lo, int(c["sexp"][k])), c0, cs))
            k += 1
    return out


def piece_value(p):
    """fp32 value of a piece: an fp32 tensor as it is, a :class:`SplitTensor` or ``(hi, lo, sexp)`` as ``SplitTensor.float()`` forms it"""
    if torch.is_tensor(p):
        return p
    if isinstance(p, tuple):
        hi, lo, sexp = p
        return (hi.float() + lo.float()) * torch.exp2(-torch.tensor([sexp], dtype=torch.int32).float())
    return p.float()


def vjp_reference(pieces, R, Ct, mutant=None):
    """``dst`` ``[R, Ct]``: per column the value of the first listed piece that covers it plus the later covering pieces in the
    listed order, in fp32; ``+0.0`` where none covers (the rule of lk_slice_vjp_f32).  MUTANTS: ``"no-zero-fill"`` leaves what was
    in memory (``FILL``) where no piece covers, ``"ignore-c0"`` puts every piece at column 0, ``"reversed"`` sums in the reverse
    order."""
    pieces = list(pieces)
    dev = next((piece_value(p).device for p, _, _ in pieces), "cpu")
    out = torch.full((R, Ct), FILL if mutant == "no-zero-fill" else 0.0, dtype=torch.float32, device=dev)
    have = torch.zeros(Ct, dtype=torch.bool, device=dev)
    for p, c0, cs in (pieces[::-1] if mutant == "reversed" else pieces):
        c0 = 0 if mutant == "ignore-c0" else c0
        v = piece_value(p).reshape(R, cs)
        seg, h = out[:, c0:c0 + cs], have[c0:c0 + cs]
        out[:, c0:c0 + cs] = torch.where(h, seg + v, v)  # (the first covering piece as it is: a -0.0 stays one)
        have[c0:c0 + cs] = True
    return out


def forward_reference(src, c0, cs):
    """columns ``[c0, c0 + cs)`` of the ``[R, Ct]`` matrix as a contiguous ``[R, cs]`` (the rule of lk_slice_fwd_f32)"""
    return src[:, c0:c0 + cs].contiguous()


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
# A CSPNetSmall of widths 64 / 64 (halves of 32 channels: the split sweep wants multiples of 32) and one block per stage,
# 8 x 8 inputs, B = 4; a ViTClassToken of dim 32, four patches and the class token (T = 5), B = 3.  Tanh / GELU networks: nothing
# is decided by a sign, so fp32 against float64 holds at the project's 1e-4 without a lattice.
E2E_CLASSES = 5


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


def _seeded(seed, build):
    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = build().double().eval()
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.7, 1.3), mod.bias.data.normal_(0, 0.2)
        return m
    finally:
        torch.random.set_rng_state(prev)


def csp_fixture(widths=(64, 64), depth=1, B=4, hw=8, classes=E2E_CLASSES, seed=31):
    """``(float64 CPU model, X, y)``: a small CSPNetSmall (tanh), deterministic"""
    from laplace_amd.nets import CSPNetSmall

    m = _seeded(seed, lambda: CSPNetSmall(classes, widths=widths, depth=depth, act=nn.Tanh))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, hw, hw, generator=gen).double(), torch.randint(classes, (B,), generator=gen)


def vit_fixture(dim=32, depth=1, heads=2, B=3, classes=E2E_CLASSES, seed=32):
    """``(float64 CPU model, X, y)``: a small ViTClassToken (8 x 8 images in four patches: T = 5 with the class token)"""
    from laplace_amd.nets import ViTClassToken

    m = _seeded(seed, lambda: ViTClassToken(classes, image=8, patch=4, dim=dim, depth=depth, heads=heads))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, 8, 8, generator=gen).double(), torch.randint(classes, (B,), generator=gen)


def taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}


class _Loader(list):
    pass


def run_curvature_checks(dev, fixture, configure=None, want_split=True, lik="classification"):
    """jacobians, diag, a two-minibatch kron fit and the Kron predictive of a fixture ``(m64, X64, y64)`` against the fp64 oracle
    at the project's tolerances (as tests/cat_fixtures.run_curvature_checks), and the proof that a SWEEP produced them (the split
    sweep when ``want_split``).  ``configure(backend)`` sets switches on every backend object; returns what routes are compared by."""
    import copy

    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep
    from oracle import curvature_oracle as co
    from tests.cat_fixtures import functional_variance_kron

    m64, X64, y64 = fixture
    n, half = X64.shape[0], (X64.shape[0] + 1) // 2
    model, X, y = copy.deepcopy(m64).float().to(dev), X64.float().to(dev), y64.to(dev)
    Js64, f64 = co.jacobians(m64, X64)
    Hl = co.functional_hessian(f64, lik)
    configure = configure or (lambda b: None)

    def swept(backend):
        tape = backend._tape()
        assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason
        sweep = getattr(tape, "sweep", None)
        assert sweep not in (None, False), "no sweep was built"
        if want_split:
            assert isinstance(sweep, SplitSweep) and sweep.split_ok, getattr(sweep, "split_reason", None)
        else:
            assert not getattr(sweep, "split_ok", False)

    backend = HipGGN(model, lik)
    configure(backend)
    Js, f = backend.jacobians(X)
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4, (rel(f, f64), rel(Js, Js64))
    _, h = backend.diag(X, y)
    assert rel(h, co.ggn_diag(Js64, Hl)) < 1e-4
    swept(backend)
    loader = _Loader([(X[:half], y[:half]), (X[half:], y[half:])])
    loader.dataset = range(n)
    la = HipLaplace(model, lik, "all", "kron", prior_precision=0.7)
    configure(la.backend)
    la.fit(loader)
    want = None
    for xb, yb in ((X64[:half], y64[:half]), (X64[half:], y64[half:])):
        _, kf = co.kfac_ggn(m64, xb, yb, n, lik)
        want = kf if want is None else co.kron_add(want, kf)
    for F_, G_ in zip(la.H_facs.kfacs, want):
        for a_, w_ in zip(F_, G_):
            assert rel(a_, w_) < 1e-4, rel(a_, w_)
    swept(la.backend)
    _, f_var = la._glm_predictive_distribution(X)
    Qs, ls = co.kron_decompose(want)
    assert rel(f_var, functional_variance_kron(Js64, Qs, ls, 0.7)) < 1e-4
    return dict(Js=Js, f=f, h=h, f_var=f_var, kfacs=[t for F_ in la.H_facs.kfacs for t in F_])
