"""TEST INFRASTRUCTURE for 1-D convolutional networks: the case table and the stated references of csrc/lk_reduce.hip (the maximum
over positions and its VJP for all seeds), and the end-to-end fixtures - a tiny ResNet1d and a tiny TextCNN, each with its
unit-height 2-D twin (``dims=2``, the same state dict with the conv weights unsqueezed) on which the fp64 oracle's KFAC runs.

The operand of the kernels is a contiguous fp32 ``[outer][L][inner]``.  The references are written from the autograd rules they
replace: ``max(dim)`` and the adaptive max pools send the cotangent to the FIRST maximum, ``amax`` splits it evenly over the maxima;
``0.0 == -0.0``.
"""
import copy

import torch
from torch import nn

GAP = 1e-3  # of the map's maximum (that of tests/cat_fixtures.py): between the largest and the second largest entry of a maximum


# ---- kernel cases ----------------------------------------------------------------------------------------------------------------
def _case(outer, L, inner, S=2, fill="random", off=0, huge=False):
    return dict(outer=outer, L=L, inner=inner, S=S, fill=fill, off=off, huge=huge)


# fill: "random" (distinct values), "first" / "last" (the maximum at position 0 / L - 1), "twice" (the maximum repeated at two
# positions), "all" (every position holds it), "negzero" (-0.0 before 0.0, both the maximum), "neginf" (a row of -inf)
CASES = [_case(o, L, i, S) for o, L, i, S in (
    (1, 1, 1, 1), (3, 2, 1, 2), (3, 63, 1, 9), (257, 64, 1, 2), (3, 65, 1, 2), (3, 257, 1, 2), (1, 64, 1, 1),  # the row path
    (1, 1, 3, 1), (3, 2, 3, 2), (3, 63, 4, 9), (1, 64, 8, 2), (3, 65, 65, 2), (257, 2, 3, 1), (3, 257, 4, 2), (257, 3, 8, 2))]
CASES += [_case(3, 65, i, 2, fill) for i in (1, 3, 4) for fill in ("first", "last", "twice", "all", "negzero", "neginf")]
CASES += [_case(3, 2, 1, 2, "twice"), _case(3, 1, 4, 2, "all")]
CASES += [_case(3, 5, 1, 2), _case(3, 9, 1, 2), _case(3, 17, 1, 2)]  # lane groups of 8, 16 and 32 on the row path
CASES += [_case(3, 64, 1, 2, off=1), _case(3, 63, 4, 2, off=1), _case(3, 8, 8, 9, off=3)]  # an unaligned base
CASES += [_case(0, 5, 1, 2), _case(0, 5, 4, 2)]  # no rows at all
# one lane past a full stride of the grid (2048 workgroups of 256 threads) on each path: the row path of the forward with 64 lanes
# per row (4 rows a workgroup), the column paths of the forward and the paths of the VJP with one element or one vector per lane
CASES += [_case(2048 * 4 + 1, 33, 1, 1), _case(2048 * 256 + 1, 1, 1, 1), _case(2048 * 256 + 1, 4, 1, 1),
          _case(2048 * 256 // 3 + 1, 1, 3, 1), _case(2048 * 256 + 1, 1, 4, 1)]
# past 2^31 elements: through lk_reduce_variant only, never run
CASES += [_case(1 << 21, 1025, 1, 1, huge=True), _case(1 << 21, 1 << 8, 4, 1, huge=True), _case(3, 1 << 29, 3, 1, huge=True),
          _case(1 << 22, 1 << 11, 1, 2, huge=True)]


def case_id(c):
    return f"o{c['outer']}-L{c['L']}-i{c['inner']}-S{c['S']}-{c['fill']}" + (f"-off{c['off']}" if c["off"] else "") + \
        ("-huge" if c["huge"] else "")


def runnable(cases=None):
    return [c for c in (CASES if cases is None else cases) if not c["huge"]]


def aligned(c):
    """are the buffers `make_operands` cuts for the case 16-byte aligned?"""
    return c["off"] % 4 == 0


def make_x(c, gen):
    """the operand ``[outer, L, inner]`` (fp32, CPU) of a case"""
    o, L, i = c["outer"], c["L"], c["inner"]
    x = torch.rand(o, L, i, generator=gen) * 2 - 1  # in (-1, 1): distinct with overwhelming probability
    fill = c["fill"]
    if fill == "first":
        x[:, 0] = 2.0
    elif fill == "last":
        x[:, L - 1] = 2.0
    elif fill == "twice":
        x[:, L // 3], x[:, L - 1] = 2.0, 2.0
    elif fill == "all":
        x[:] = 0.75
    elif fill == "negzero":
        x = -x.abs() - 0.5
        x[:, L // 3], x[:, L // 2 + 1] = -0.0, 0.0
    elif fill == "neginf":
        x[:] = float("-inf")
    return x.float()


def forward_reference(x, mutant=None):
    """``(y, idx, cnt)``: the maximum over dim 1 of ``x [outer, L, inner]``, the first position that holds it and the number of
    positions that compare equal to it (int32).  ``mutant="last"``: the last position instead of the first."""
    o, L, i = x.shape
    y = x.amax(1) if o and i else x.new_empty(o, i)
    eq = x == y.unsqueeze(1)
    pos = torch.arange(L, dtype=torch.int32).reshape(1, L, 1).expand(o, L, i)
    if mutant == "last":
        idx = torch.where(eq, pos, torch.full_like(pos, -1)).amax(1) if o and i else pos.new_empty(o, i)
    else:
        idx = torch.where(eq, pos, torch.full_like(pos, L)).amin(1) if o and i else pos.new_empty(o, i)
    return y, idx.to(torch.int32), eq.sum(1).to(torch.int32)


def vjp_reference(g, x, even, mutant=None, into=None):
    """``dx [S, outer, L, inner]`` (fp64) for ``g [S, outer, inner]``: first mode ``(l == idx) ? g : 0``, even mode
    ``(x == y) ? g / cnt : 0`` with the exact quotient.  Mutants: ``"last"`` (the last maximum), ``"first-for-amax"`` (the even mode
    answered with the first maximum), ``"no-fill"`` (the elements off the maximum keep what ``into`` held: the zero fill skipped)."""
    S = g.shape[0]
    o, L, i = x.shape
    y, idx, cnt = forward_reference(x, "last" if mutant == "last" else None)
    pos = torch.arange(L, dtype=torch.int32).reshape(1, L, 1)
    if even and mutant != "first-for-amax":
        hit, q = x == y.unsqueeze(1), g.double() / cnt.double()
    else:
        hit, q = pos == idx.unsqueeze(1), g.double()
    rest = torch.zeros(S, o, L, i, dtype=torch.float64) if mutant != "no-fill" else into.double()
    return torch.where(hit.unsqueeze(0), q.unsqueeze(2).expand(S, o, L, i), rest)


def even_bound(g, x):
    """per element: what one fp32 division that need not be correctly rounded may miss the fp64 quotient by, ``2^-23 |g / cnt|``"""
    _, _, cnt = forward_reference(x)
    return (2.0 ** -23 * (g.double() / cnt.double().clamp(min=1)).abs()).unsqueeze(2)


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
E2E_CLASSES = 3


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


def twin_of(model, build2d):
    """the ``dims=2`` twin with the state dict of ``model`` (conv weights unsqueezed at dim 2) and the same tracked parameters"""
    twin = build2d().to(next(model.parameters()).dtype).eval()
    sd = {k: (v.unsqueeze(2) if v.dim() == 3 and k.endswith("weight") and twin.state_dict()[k].dim() == 4 else v)
          for k, v in model.state_dict().items()}
    twin.load_state_dict(sd)
    for (_, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        q.requires_grad_(p.requires_grad)
    return twin


def _seeded(seed, build):
    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = build().double().eval()
        for mod in m.modules():
            if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
                mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.7, 1.3), mod.bias.data.normal_(0, 0.2)
        return m
    finally:
        torch.random.set_rng_state(prev)


def _gaps(model, X):
    """the relative gap (largest minus second largest entry, over the map's max |.|) of every max window and max reduction"""
    gaps, hooks = [], []

    def windows(x, k, s, p, d):
        xp = nn.functional.pad(x, (p, p), value=float("-inf"))
        L = xp.shape[-1]
        n = (L - d * (k - 1) - 1) // s + 1
        return torch.stack([xp[..., j * s:j * s + d * (k - 1) + 1:d] for j in range(n)], -2)  # [.., n, k]

    def gap_of(w, scale):
        top = w.topk(2, -1).values if w.shape[-1] > 1 else None
        if top is not None:
            fin = torch.isfinite(top[..., 1])
            gaps.append(((top[..., 0] - top[..., 1])[fin] / scale).min().item())

    def pool_hook(m, inp, out):
        x = inp[0]
        x = x.squeeze(2) if x.dim() == 4 else x
        one = lambda v: v[-1] if isinstance(v, (tuple, list)) else v
        gap_of(windows(x, one(m.kernel_size), one(m.stride), one(m.padding), one(m.dilation)), x.abs().max())

    for mod in model.modules():
        if isinstance(mod, (nn.MaxPool1d, nn.MaxPool2d)):
            hooks.append(mod.register_forward_hook(pool_hook))
        if isinstance(mod, nn.ModuleList) and hasattr(model, "acts") and mod is model.acts:
            for a in mod:  # (TextCNN: every activation feeds an amax over the positions)
                hooks.append(a.register_forward_hook(lambda m, i, o: gap_of(o.flatten(2), o.abs().max())))
    with torch.no_grad():
        model(X)
    for h in hooks:
        h.remove()
    return gaps


def resnet1d_fixture(freeze_depthwise=False, seed=41, B=3, L=16):
    """``(float64 CPU model, its 2-D twin, X [B, 2, L], X of the twin, y)``: a tiny ResNet1d - widths 4 / 8, one block per stage,
    tanh, a strided convolution with dilation 2 and depthwise second convolutions - calibrated so that every max-pool window
    keeps `GAP` (asserted by tests/test_conv1d_fixtures.py)"""
    from laplace_amd.nets import ResNet1d

    build = lambda dims: ResNet1d(E2E_CLASSES, 2, (4, 8), 1, nn.Tanh, True, dims, dilation=2, depthwise=True,
                                  freeze_depthwise=freeze_depthwise)
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(E2E_CLASSES, (B,), generator=gen)
    for attempt in range(64):  # (deterministic: the first seed whose fp64 forward keeps the gap)
        m = _seeded(seed + 100 * attempt, lambda: build(1))
        X = torch.randn(B, 2, L, generator=gen).double()
        if min(_gaps(m, X)) >= 4 * GAP:
            break
    return m, twin_of(m, lambda: build(2)), X, X.unsqueeze(2), y


def textcnn_fixture(seed=43, B=3, T=9):
    """``(float64 CPU model, its 2-D twin, token ids [B, T], the same, y)``: a tiny TextCNN (vocabulary 11, embedding 6, 5 channels
    per width, GELU), calibrated so that every maximum over the positions keeps `GAP`"""
    from laplace_amd.nets import TextCNN

    build = lambda dims: TextCNN(E2E_CLASSES, 11, 6, 5, (3, 4, 5), nn.GELU, True, dims)
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(E2E_CLASSES, (B,), generator=gen)
    for attempt in range(64):
        m = _seeded(seed + 100 * attempt, lambda: build(1))
        X = torch.randint(11, (B, T), generator=gen)
        if min(_gaps(m, X)) >= 4 * GAP:
            break
    return m, twin_of(m, lambda: build(2)), X, X, y


FIXTURES = {"resnet1d": lambda: resnet1d_fixture(freeze_depthwise=True), "resnet1d-dw": resnet1d_fixture, "textcnn": textcnn_fixture}


class _Loader(list):
    pass


def run_curvature_checks(dev, fixture, configure=None, kron=True, lik="classification"):
    """f, jacobians, diag, full, a two-minibatch kron fit and the Kron and diagonal GLM predictive of a fixture against the fp64
    oracle at the project's tolerances; the KFAC factors are the oracle's ON THE TWIN (``oracle.kfac_ggn`` knows nn.Conv2d), held
    element-wise to ``1e-4 |b| + 1e-6 max|b|``.  ``configure(backend)`` sets switches on every backend object.  Returns the
    quantities and the worst error / bound ratios."""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co
    from tests.cat_fixtures import functional_variance_kron

    m64, twin, X64, X2, y64 = fixture
    n, half = X64.shape[0], (X64.shape[0] + 1) // 2
    model, y = copy.deepcopy(m64).float().to(dev), y64.to(dev)
    X = (X64.float() if X64.is_floating_point() else X64).to(dev)
    Js64, f64 = co.jacobians(m64, X64)
    Hl = co.functional_hessian(f64, lik)
    configure = configure or (lambda b: None)
    ratios = {}
    backend = HipGGN(model, lik)
    configure(backend)
    assert backend._supported()
    Js, f = backend.jacobians(X)
    ratios["f"], ratios["Js"] = rel(f, f64) / 1e-5, rel(Js, Js64) / 1e-4
    assert ratios["f"] < 1 and ratios["Js"] < 1, ratios
    _, h = backend.diag(X, y)
    ratios["diag"] = rel(h, co.ggn_diag(Js64, Hl)) / 1e-4
    _, H = backend.full(X, y)
    ratios["full"] = rel(H, co.ggn_full(Js64, Hl)) / 1e-4
    assert ratios["diag"] < 1 and ratios["full"] < 1, ratios
    out = dict(Js=Js, f=f, h=h, H=H, backend=backend)
    la = HipLaplace(model, lik, "all", "diag", prior_precision=0.7)
    configure(la.backend)
    loader = _Loader([(X[:half], y[:half]), (X[half:], y[half:])])
    loader.dataset = range(n)
    la.fit(loader)
    _, dvar = la._glm_predictive_distribution(X)
    post = 1.0 / (co.ggn_diag(Js64, Hl) + 0.7)
    want_d = torch.einsum("ncp,p,nkp->nck", Js64, post, Js64)
    ratios["diag-predictive"] = rel(dvar, want_d) / 1e-4
    assert ratios["diag-predictive"] < 1, ratios
    out["dvar"] = dvar
    if kron:
        la = HipLaplace(model, lik, "all", "kron", prior_precision=0.7)
        configure(la.backend)
        la.fit(loader)
        want = None
        for xb, yb in ((X2[:half], y64[:half]), (X2[half:], y64[half:])):
            _, kf = co.kfac_ggn(twin, xb, yb, n, lik)
            want = kf if want is None else co.kron_add(want, kf)
        worst = 0.0
        for F_, G_ in zip(la.H_facs.kfacs, want):
            for a_, w_ in zip(F_, G_):
                a_, w_ = a_.detach().double().cpu(), w_.double()
                assert a_.shape == w_.shape, (a_.shape, w_.shape)
                worst = max(worst, ((a_ - w_).abs() / (1e-4 * w_.abs() + 1e-6 * w_.abs().max())).max().item())
        ratios["kron"] = worst
        assert worst < 1, worst
        _, f_var = la._glm_predictive_distribution(X)
        Qs, ls = co.kron_decompose(want)
        ratios["kron-predictive"] = rel(f_var, functional_variance_kron(Js64, Qs, ls, 0.7)) / 1e-4
        assert ratios["kron-predictive"] < 1, ratios
        out.update(f_var=f_var, kfacs=[t for F_ in la.H_facs.kfacs for t in F_], la=la)
    out["ratios"] = ratios
    return out
