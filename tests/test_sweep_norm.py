"""GroupNorm and LayerNorm in the seed-batched reverse sweep (laplace_amd/sweep.py, sweep_nhwc.py) - host logic with
``kernels=None`` (plain torch math) and on the kernel emulation with the two norm entry points
(tests/emulated_normvjp_kernels.py), against one autograd pass per seed at ``rtol=1e-4, atol=1e-7`` as tests/test_sweep_rules.py.

Before the rule existed every sweep constructed here raised ``SweepUnsupported("no VJP rule for module GroupNorm ...")``.
"""
import pytest
import torch
from torch import nn

from laplace_amd.sweep import NORM, SeedBatchedSweep, SweepUnsupported
from tests.norm_fixtures import build_model, golden_model, input_shape, load_golden, n_outputs, rel
from tests.norm_sweep_fixtures import autograd_reference as _autograd_reference

TOL = 1e-5  # (of tests/test_norm_params.py: the emulation is stock torch)


@pytest.fixture
def normvjp_kernels():
    from laplace_amd import _lib
    from tests.emulated_normvjp_kernels import EmulatedNormVjpKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormVjpKernels())
    yield
    _lib.set_kernels_for_testing(prev)


class _GNResBlock(nn.Module):
    """``_BNResBlock`` of tests/norm_fixtures.py with GroupNorm(2, c) in the BatchNorm positions"""

    def __init__(self, c, **kw):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 3, padding=1, bias=False)
        self.bn1 = nn.GroupNorm(2, c, **kw)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(c, c, 3, padding=1, bias=False)
        self.bn2 = nn.GroupNorm(2, c, **kw)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += identity
        return self.relu(out)


def _stir(model):
    for m in model.modules():
        if isinstance(m, (nn.GroupNorm, nn.LayerNorm)) and m.weight is not None:
            m.weight.data.uniform_(-1.5, 1.5)
            m.bias.data.normal_(0.0, 0.3)
    return model.eval()


def _gn_net(groups, **kw):
    return nn.Sequential(nn.Conv2d(2, 8, 3, padding=1), nn.GroupNorm(groups, 8, **kw), nn.Tanh(), nn.AdaptiveAvgPool2d(1),
                         nn.Flatten(), nn.Linear(8, 3))


MODELS = {
    "normgn": lambda: (build_model("normgn"), input_shape("normgn"), n_outputs("normgn")),
    "normln": lambda: (build_model("normln"), input_shape("normln"), n_outputs("normln")),
    "gn-residual": lambda: (nn.Sequential(nn.Conv2d(2, 8, 3, padding=1), _GNResBlock(8), _GNResBlock(8), nn.AdaptiveAvgPool2d(1),
                                          nn.Flatten(), nn.Linear(8, 3)), (2, 5, 5), 3),
    "gn-8-of-8": lambda: (_gn_net(8), (2, 4, 4), 3),
    "gn-1-of-8": lambda: (_gn_net(1), (2, 4, 4), 3),
    "gn-no-affine": lambda: (_gn_net(2, affine=False), (2, 4, 4), 3),
    "ln-no-affine": lambda: (nn.Sequential(nn.Linear(5, 8), nn.LayerNorm(8, elementwise_affine=False), nn.Tanh(), nn.Flatten(),
                                           nn.Linear(32, 2)), (4, 5), 2),
    # an in-place op behind a layer WITHOUT affine parameters writes into the layer's output, which must not be the kept xhat
    "gn-no-affine-inplace-relu": lambda: (nn.Sequential(nn.Conv2d(2, 8, 3, padding=1), nn.GroupNorm(2, 8, affine=False),
                                                        nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                                                        nn.Linear(8, 3)), (2, 4, 4), 3),
    "ln-no-affine-inplace-relu": lambda: (nn.Sequential(nn.Linear(5, 8), nn.LayerNorm(8, elementwise_affine=False),
                                                        nn.ReLU(inplace=True), nn.Flatten(), nn.Linear(32, 2)), (4, 5), 2),
    "gn-no-affine-residual": lambda: (nn.Sequential(nn.Conv2d(2, 8, 3, padding=1), _GNResBlock(8, affine=False),
                                                    _GNResBlock(8, affine=False), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                                                    nn.Linear(8, 3)), (2, 5, 5), 3),  # (``out += identity`` behind bn2)
    "ln-two-dims": lambda: (nn.Sequential(nn.Linear(5, 6), nn.LayerNorm((4, 6)), nn.Sigmoid(), nn.Flatten(), nn.Linear(24, 2)),
                            (4, 5), 2),
}


def _taps(model, with_norm):
    kinds = (nn.Conv2d, nn.Linear) + ((nn.GroupNorm, nn.LayerNorm) if with_norm else ())
    return {n: m for n, m in model.named_modules() if isinstance(m, kinds)}


def _compare(model, shape, C, kernels, with_norm=False, cls=SeedBatchedSweep):
    torch.manual_seed(3)
    x, seeds = torch.randn(3, *shape), torch.randn(4, 3, C)
    taps = _taps(model, with_norm)
    sw = cls(model, taps, kernels=kernels)
    assert any(r.kind == NORM for r in sw.rule.values())
    f = sw.forward(x)
    grads = sw.backward(seeds)
    f_ref, ins, want = _autograd_reference(model, taps, x, seeds)
    assert torch.allclose(f, f_ref, rtol=1e-4, atol=1e-7)
    for n in taps:
        assert torch.allclose(sw.taps[n]["a"], ins[n], rtol=1e-4, atol=1e-7), n
        assert grads[n].shape == want[n].shape, n
        assert torch.allclose(grads[n], want[n], rtol=1e-4, atol=1e-7), (n, (grads[n] - want[n]).abs().max().item())
    return sw


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_in_plain_torch_against_one_autograd_pass_per_seed(name):
    torch.manual_seed(len(name))
    model, shape, C = MODELS[name]()
    _compare(_stir(model), shape, C, None)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_on_the_emulated_kernels_against_one_autograd_pass_per_seed(normvjp_kernels, name, monkeypatch):
    from laplace_amd._lib import get_kernels

    calls = []
    K = get_kernels()
    for what in ("norm_forward", "norm_vjp"):
        inner = getattr(K, what)
        monkeypatch.setattr(K, what, lambda *a, _i=inner, _w=what, **kw: (calls.append(_w), _i(*a, **kw))[1], raising=False)
    torch.manual_seed(len(name))
    model, shape, C = MODELS[name]()
    sw = _compare(_stir(model), shape, C, get_kernels)
    n_norm = sum(r.kind == NORM for r in sw.rule.values())
    # one forward launch per norm node; one VJP launch for ALL seeds per norm node (the first node of `normln` sits behind a
    # tapped Linear, which is where the sweep stops - every norm node here has a tapped layer upstream)
    assert calls.count("norm_forward") == n_norm and calls.count("norm_vjp") == n_norm, calls


@pytest.mark.parametrize("name", ("normgn", "normln", "gn-residual"))
@pytest.mark.parametrize("emulated", (False, True))
def test_tapped_norm_layers_get_their_output_cotangent_and_input(name, emulated, request):
    """a tapped GroupNorm / LayerNorm: the cotangent of its OUTPUT and its input ``a`` are the tape's"""
    if emulated:
        request.getfixturevalue("normvjp_kernels")
    from laplace_amd._lib import get_kernels

    torch.manual_seed(7)
    model, shape, C = MODELS[name]()
    sw = _compare(_stir(model), shape, C, get_kernels if emulated else None, with_norm=True)
    assert any(isinstance(sw.modules[n], (nn.GroupNorm, nn.LayerNorm)) for n in sw.taps)


def test_functional_spellings_stay_refused():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc, self.ln = nn.Linear(4, 6), nn.LayerNorm(6)

        def forward(self, x):
            return torch.nn.functional.layer_norm(self.fc(x), (6,), self.ln.weight, self.ln.bias)

    m = M().eval()
    with pytest.raises(SweepUnsupported):
        SeedBatchedSweep(m, {"fc": m.fc})


@pytest.mark.parametrize("emulated", (False, True))
def test_forward_without_vjp_keeps_nothing(emulated, request):
    if emulated:
        request.getfixturevalue("normvjp_kernels")
    from laplace_amd._lib import get_kernels

    model, shape, C = MODELS["gn-residual"]()
    model = _stir(model)
    sw = SeedBatchedSweep(model, _taps(model, False), kernels=get_kernels if emulated else None)
    x = torch.randn(2, *shape)
    f = sw.forward(x, need_vjp=False)
    assert sw.saved == {}
    assert torch.allclose(f, model(x), rtol=1e-4, atol=1e-7)
    sw.forward(x)
    assert sum(sw.rule[n].kind == NORM for n in sw.saved) == 4


# ---- through the backend --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ("classification", "regression"))
@pytest.mark.parametrize("name", ("normgn", "normln"))
def test_backend_sweeps_the_norm_models_and_meets_the_goldens(normvjp_kernels, monkeypatch, name, lik):
    """``jacobians`` and ``diag`` at the ``TOL`` of tests/test_norm_params.py, on the sweep: the sweep of route ``{"norm"}`` is a
    sweep object (it was ``False``: the model dropped to one autograd pass per seed) and ``torch.autograd.grad`` is never called"""
    from laplace_amd import HipGGN

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g)
    b = HipGGN(model, lik)
    real, calls = torch.autograd.grad, []
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    Js, f = b.jacobians(X)
    loss, h = b.diag(X, y)
    monkeypatch.setattr(torch.autograd, "grad", real)
    assert not calls, f"{len(calls)} autograd passes"
    tape = b._tape()
    assert isinstance(tape.sweeps.get(frozenset({"norm"})), SeedBatchedSweep), getattr(tape, "sweep_reason", None)
    for got, want, what in ((Js, g["Js"], "jacobians"), (f, g["f"], "f"), (h, g["h_ggn"], "diag GGN"), (loss, g["loss"], "loss")):
        e = rel(got, want)
        print(f"{name} {lik} {what}: {e:.3e}")
        assert e < TOL, f"{what}: rel err {e:.3e}"


# ---- eligibility of the NHWC split sweep ------------------------------------------------------------------------------------
def _split_net(kind):
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(32, 32, 3, 1, 1, bias=False)
            self.n1 = nn.LayerNorm((32, 4, 4)) if kind == "ln-on-map" else nn.GroupNorm(8, 32)
            self.c2 = nn.Conv2d(32, 32, 3, 1, 1, bias=False)
            self.pool, self.flat = nn.AdaptiveAvgPool2d(1), nn.Flatten()
            self.fc1, self.ln, self.fc = nn.Linear(32, 16), nn.LayerNorm(16), nn.Linear(16, 3)

        def forward(self, x):
            h = torch.tanh(self.n1(self.c1(x)))
            h = self.flat(self.pool(torch.relu(self.c2(h))))
            return self.fc(torch.tanh(self.ln(self.fc1(h))))

    return M().eval()


@pytest.mark.parametrize("kind,tap_norm,fragment", [
    ("gn", False, None),  # untapped GroupNorm on a feature map, LayerNorm in the head region: eligible
    ("gn", True, "n1: tapped GroupNorm"),
    ("ln-on-map", False, "n1: LayerNorm applied to a feature map"),
])
def test_split_sweep_eligibility_is_decided_on_the_graph(normvjp_kernels, kind, tap_norm, fragment):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(2)
    model = _split_net(kind)
    taps = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    if tap_norm:
        taps["n1"] = model.n1
    sw = SplitSweep(model, taps, kernels=get_kernels)
    if fragment is None:
        assert sw.split_ok, sw.split_reason
    else:
        assert not sw.split_ok and fragment in sw.split_reason, sw.split_reason


@pytest.mark.parametrize("missing", ("norm_forward", "norm_vjp"))
def test_split_sweep_wants_both_norm_entry_points(normvjp_kernels, missing):
    """the forward calls ``norm_forward`` and the backward ``norm_vjp``: a kernel object without either makes the model
    ineligible before anything runs"""
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    def absent(self):
        raise AttributeError(missing)

    K = type("OneEntryPoint", (type(get_kernels()),), {missing: property(absent)})()
    assert not hasattr(K, missing)
    model = _split_net("gn")
    taps = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    sw = SplitSweep(model, taps, kernels=lambda: K)
    assert not sw.split_ok and "n1: kernels without the per-sample normalisation entry points" in sw.split_reason


def test_split_sweep_runs_groupnorm_on_nhwc_and_the_head_layernorm_in_the_parent(normvjp_kernels, monkeypatch):
    """the eligible net of the test above through the split sweep on the emulation: both norm nodes served, GroupNorm in layout 1
    with a max|dx| word, against one autograd pass per seed (split-fp16 cotangents: 1e-4 max-normalised)"""
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(2)
    model = _split_net("gn")
    model.n1.weight.data.uniform_(-1.5, 1.5)
    taps = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    K, seen = get_kernels(), []
    inner = K.norm_vjp
    monkeypatch.setattr(K, "norm_vjp", lambda *a, **kw: (seen.append((a[6], kw.get("amax") is not None)), inner(*a, **kw))[1],
                        raising=False)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    x, seeds = torch.randn(3, 32, 4, 4), torch.randn(2, 3, 3)
    f = sw.forward(x)
    grads = sw.backward(seeds)
    assert sorted(seen) == [(1, False), (1, True)], seen  # (head LayerNorm: layout 1 without a word; GroupNorm: NHWC with one)
    f_ref, _, want = _autograd_reference(model, taps, x, seeds)
    assert torch.allclose(f, f_ref, rtol=1e-3, atol=1e-5)
    for n in taps:
        got = grads[n]
        assert got.shape == want[n].shape, (n, got.shape, want[n].shape)
        assert rel(got, want[n]) < 1e-4, n
