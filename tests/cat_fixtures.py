"""Shapes, inputs and references for the concatenation kernels (csrc/lk_cat.hip) and the small DenseNets of the end-to-end tests -
shared by tests/test_cat_fixtures.py (CPU: the table reaches every path, the references bite, the ReLU fixture decides clear of
near ties) and tests/test_gpu_cat.py (the device).

A kernel case is a dict: rows ``R``, channels of the parts ``Ct``, the slice ``c0`` / ``Cs``, ``kinds`` (per part ``"f32"`` or
``"split"``, in the listed order), ``sexp`` (per split part), ``off`` (1: every buffer starts one element past an aligned
address) and ``huge`` (the part alone is larger than 2^31 elements: device only).  The shapes are the smallest at which a path
can go wrong: one row, one short of / at / one past a wave, more than one workgroup, one row past a full stride of the grid
(2048 workgroups of 256 lanes) on the vector and on the scalar path, slices that are and are not multiples of four channels at
offsets that are and are not, a slice that is the whole map and one inside a wider map, unaligned bases, no rows at all, and
one to four parts of every mix.
"""
import torch
from torch import nn

GRID_LANES = 2048 * 256  # lanes of one stride of the grid (CAT_MAX_BLOCKS x 256 of csrc/lk_cat.hip)
MAX_PARTS = 4


def _case(R, c0, Cs, extra=0, kinds=("f32",), sexp=(3, -2, 0, 7), off=0, huge=False):
    return dict(R=R, Ct=c0 + Cs + extra, c0=c0, Cs=Cs, kinds=tuple(kinds), sexp=tuple(sexp[:len(kinds)]), off=off, huge=huge)


_MIXES = [("f32",), ("split",), ("f32", "split"), ("split", "f32"), ("split", "split"), ("f32", "f32"), ("f32", "split", "f32"),
          ("split", "split", "split"), ("f32", "f32", "f32"), ("split", "f32", "split", "f32"), ("f32", "f32", "f32", "f32"),
          ("split", "split", "split", "split"), ("f32", "split", "split", "f32")]
_RS, _CSS, _C0S = (1, 63, 64, 65, 257), (1, 3, 4, 8, 32, 36), (0, 3, 4, 32)

CASES = []
_n = 0
for _Cs in _CSS:
    for _c0 in _C0S:
        # every (Cs, c0) with Ct = c0 + Cs and with a wider map; R, the mix of parts and the alignment rotate through their values
        for _extra in (0, 4 if (_Cs + _c0) % 2 == 0 else 5):
            CASES.append(_case(_RS[_n % 5], _c0, _Cs, _extra, _MIXES[_n % len(_MIXES)], off=int(_n % 5 == 2)))
            _n += 1
CASES += [
    # every mix on the vector path and on the scalar path, over more than one workgroup
    *[_case(257, 4, 8, 4, mix) for mix in _MIXES], *[_case(65, 3, 3, 1, mix, off=i % 2) for i, mix in enumerate(_MIXES)],
    # an unaligned base with a shape that would otherwise take 16-byte accesses
    _case(64, 32, 32, 0, ("f32", "split"), off=1), _case(257, 0, 4, 4, ("split",), off=1),
    # one row past a full stride of the grid: one lane per row on the vector path (Cs = 4) and on the scalar path (Cs = 1)
    _case(GRID_LANES + 1, 4, 4, 0, ("f32", "split")), _case(GRID_LANES + 1, 3, 1, 0, ("split", "f32", "f32")),
    # no rows
    _case(0, 4, 8, 4, ("f32", "split")),
    # the element index of the part passes 2^31 (R * Ct = 2^31 + 4 * 2052 + ...): the offsets are 64-bit
    _case((1 << 20) + 3, 2048, 4, 0, ("f32",), huge=True),
]


def case_id(c):
    return (f"R{c['R']}-Ct{c['Ct']}-c{c['c0']}+{c['Cs']}-" + "".join("s" if k == "split" else "f" for k in c["kinds"])
            + ("-unaligned" if c["off"] else "") + ("-huge" if c["huge"] else ""))


def split_mask(c):
    return sum(1 << i for i, k in enumerate(c["kinds"]) if k == "split")


def make_parts(c, gen):
    """the parts of a case on the CPU: per part an fp32 ``[R, Ct]`` tensor, or ``(hi, lo, sexp)`` - fp16 planes ``[R, Ct]`` and an
    int - whose value is ``(float(hi) + float(lo)) * 2^-sexp``.  Finite, no integers; the scales keep every value far from the
    subnormals (|hi| <= 65504, and a half's smallest non-zero magnitude 2^-24 times 2^-7 is 2^-31)."""
    parts, k = [], 0
    for kind in c["kinds"]:
        if kind == "f32":
            parts.append(torch.randn(c["R"], c["Ct"], generator=gen) * 1.7 + 0.01)
        else:
            hi = torch.randn(c["R"], c["Ct"], generator=gen).half()
            lo = (torch.randn(c["R"], c["Ct"], generator=gen) * 2.0 ** -11).half()
            parts.append((hi, lo, int(c["sexp"][k])))
            k += 1
    return parts


def part_value(p):
    """fp32 value of a part, formed as ``SplitTensor.float()`` forms it"""
    if torch.is_tensor(p):
        return p
    hi, lo, sexp = p
    return (hi.float() + lo.float()) * torch.exp2(-torch.tensor([sexp], dtype=torch.int32).float())


def vjp_reference(c, parts, mutant=None):
    """``dst`` ``[R, Cs]``: the fp32 sum of ``value_p[:, c0:c0 + Cs]`` taken in the listed order.  MUTANTS: ``"ignore-c0"`` reads
    the slice at channel 0, ``"reversed"`` sums right to left."""
    c0 = 0 if mutant == "ignore-c0" else c["c0"]
    vals = [part_value(p)[:, c0:c0 + c["Cs"]] for p in parts]
    if mutant == "reversed":
        vals = vals[::-1]
    acc = vals[0].clone()
    for v in vals[1:]:
        acc = acc + v
    return acc


def order_matters(c):
    """a case on which another order of the sum changes bits: three or more generic parts and enough elements"""
    return len(c["kinds"]) >= 3 and c["R"] * c["Cs"] >= 64 and not c["huge"]


# ---- end-to-end fixtures: small DenseNets ----------------------------------------------------------------------------------------
# Two blocks of two layers, growth 32, 8 x 8 inputs, B = 4, five classes.  The tanh network decides nothing: generic weights,
# BatchNorm statistics away from the identity.  The ReLU network is built on the dyadic-lattice recipe of tests/pool_fixtures.py
# (integer inputs times h = 1/8, two entries of +-1 per filter of the stem and ONE per filter of every other convolution - a sum of
# two taps doubles a map's range at every layer -, BatchNorm with zero mean and running_var + eps = 1): every raw map
# (convolution output, concatenation, pooled map) holds multiples of h.  Ten ReLUs deep, a half-step offset in front of every
# ReLU would cost one bit of max / step per layer and leave less than GAP at the end, so every BatchNorm has weight 2 and a
# NEGATIVE offset -(2 m + 1) h: z = 2 x - (2 m + 1) h is an odd multiple of h (never zero, |z| >= h), the ReLU's output is 0 or an
# odd multiple of h, and the offset cuts the range from below, which keeps max|z| / h bounded at every depth.  m is calibrated per
# layer and channel on the float64 forward (the 0.7 quantile of x stays positive: three pre-activations in ten at least).  The transitions'
# convolutions have entries of +-4, so that the average over 2 x 2 stays on the lattice.  All of it is exact in fp32 and fp16.
E2E_CLASSES, E2E_B, E2E_HW = 5, 4, 8
GAP = 1e-3  # of the map's maximum
H_STEP = 0.125


def _densenet(act):
    from laplace_amd.nets import DenseNetSmall

    return DenseNetSmall(E2E_CLASSES, growth=32, blocks=(2, 2), stem=64, act=act).double().eval()


def _calibrate_offsets_(model, X, quantile=0.7):
    """set every BatchNorm's offsets to -(2 m + 1) h, m per channel, from the float64 forward (in graph order: a layer's input depends on the
    offsets of the layers before it only)"""
    def pre(bn, inp):
        x = inp[0].detach().transpose(0, 1).flatten(1)  # [C, B H W]: one offset per channel, so that no channel dies
        # (the largest m that leaves the channel's `quantile` value positive: a share of 1 - quantile at least stays alive)
        m = torch.round(torch.quantile(x, quantile, dim=1, interpolation="lower") / H_STEP) - 1
        bn.bias.data.copy_(-(2 * m + 1) * H_STEP)

    hooks = [mod.register_forward_pre_hook(pre) for mod in model.modules() if isinstance(mod, nn.BatchNorm2d)]
    with torch.no_grad():
        model(X)
    for h in hooks:
        h.remove()


def e2e_fixture(kind):
    """``(float64 CPU model, X, y)`` for ``kind`` "tanh" / "relu"; deterministic"""
    from tests.pool_fixtures import _lattice_bn_, _ternary_

    seed = {"tanh": 21, "relu": 22}[kind]
    gen = torch.Generator().manual_seed(seed)
    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)  # (the layers this function does not fill keep their constructor's values, which draw from here)
    try:
        m = _densenet(nn.Tanh if kind == "tanh" else nn.ReLU)
    finally:
        torch.random.set_rng_state(prev)
    if kind == "tanh":
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.3, generator=gen), mod.running_var.uniform_(0.5, 2.0, generator=gen)
                mod.weight.data.uniform_(0.7, 1.3, generator=gen), mod.bias.data.normal_(0, 0.2, generator=gen)
        X = torch.randn(E2E_B, 3, E2E_HW, E2E_HW, generator=gen).double()
    else:
        for name, mod in m.named_modules():
            if isinstance(mod, nn.Conv2d):
                _ternary_(mod.weight, gen, nonzero=2 if name == "conv1" else 1)
            elif isinstance(mod, nn.BatchNorm2d):
                _lattice_bn_(mod, 2.0, -H_STEP)
        for mod in m.modules():  # the transitions: entries of +-4 in front of the 2 x 2 average
            if isinstance(mod, nn.Sequential) and len(mod) and isinstance(mod[-1], nn.AvgPool2d):
                mod[2].weight.data.mul_(4.0)
        X = torch.randint(-2, 3, (E2E_B, 3, E2E_HW, E2E_HW), generator=gen).double() * H_STEP
        _calibrate_offsets_(m, X)
    y = torch.randint(E2E_CLASSES, (E2E_B,), generator=gen)
    return m, X, y


def e2e_taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}


def relu_gaps(model, X):
    """per ReLU of the float64 forward: ``(smallest |pre-activation| / largest, share of positive pre-activations, count)``"""
    out = []

    def pre(mod, inp):
        z = inp[0].detach()
        out.append(((z.abs().min() / z.abs().max()).item(), (z > 0).double().mean().item(), z.numel()))

    hooks = [mod.register_forward_pre_hook(pre) for mod in model.modules() if isinstance(mod, nn.ReLU)]
    with torch.no_grad():
        model(X)
    for h in hooks:
        h.remove()
    return out


def functional_variance_kron(Js, eigvecs, eigvals, prior_prec, h_factor=1.0):
    """``oracle.curvature_oracle.functional_variance_kron`` (no damping) block by block in the eigenbasis, WITHOUT the dense
    ``P x P`` matrix the oracle's definition-level form builds: a 3 x 3 convolution of 128 to 32 channels alone would take 10 GiB
    there.  Same decomposition, same eigenvalues (the oracle's own `_block_eigvals`), the same sum in another order;
    tests/test_cat_fixtures.py holds the two against each other on a model the dense form can take."""
    from oracle import curvature_oracle as co

    ev = co.krondecomposed_scale(eigvals, h_factor)
    deltas = co._expand_deltas(prior_prec, len(ev), ev[0][0].dtype)
    B, K, _ = Js.shape
    out, at = torch.zeros(B, K, K, dtype=Js.dtype), 0
    for Qs, ls, d in zip(eigvecs, ev, deltas):
        lam = co._block_eigvals(ls, d, False).reshape(-1)
        W = Js[:, :, at:at + lam.numel()]
        if len(Qs) == 1:
            R = W @ Qs[0]
        else:
            d0, d1 = Qs[0].shape[0], Qs[1].shape[0]
            R = torch.einsum("bkac,ai,cj->bkij", W.reshape(B, K, d0, d1), Qs[0], Qs[1]).reshape(B, K, -1)
        out += torch.einsum("bkn,n,bln->bkl", R, 1.0 / lam, R)
        at += lam.numel()
    assert at == Js.shape[2]
    return out


# ---- curvature against the oracle (the ``run_curvature_checks`` of tests/attn_fixtures.py for a convolutional model) -----------------
class _Loader(list):
    pass


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


def small_dense(C, act=nn.Tanh, seed=7):
    """``(float64 CPU model, X [6, 3, 4, 4] float64)``: a DenseNet of two blocks of one layer (stem 32, growth 32) - every piece of the
    workload (nested concatenations, an average-pool transition, pre-activation BatchNorm) at a size whose Jacobians are small"""
    from laplace_amd.nets import DenseNetSmall

    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = DenseNetSmall(C, growth=32, blocks=(1, 1), stem=32, act=act).double().eval()
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.7, 1.3), mod.bias.data.normal_(0, 0.2)
        X = torch.randn(6, 3, 4, 4, dtype=torch.float64)
    finally:
        torch.random.set_rng_state(prev)
    return m, X


def run_curvature_checks(dev, lik, configure=None, want_split=True):
    """jacobians, diag, a two-minibatch kron fit and the Kron predictive of `small_dense` against the fp64 oracle at the project's
    tolerances, and the proof that a SWEEP produced them (the split sweep when ``want_split``).  ``configure(backend)`` sets
    switches on every backend object; returns what the routes are compared by."""
    import copy

    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep
    from oracle import curvature_oracle as co

    C = 3 if lik == "classification" else 2
    m64, X64 = small_dense(C)
    model, X = copy.deepcopy(m64).float().to(dev), X64.float().to(dev)
    gen = torch.Generator().manual_seed(11)
    y64 = torch.randint(C, (6,), generator=gen) if lik == "classification" else torch.randn(6, C, generator=gen).double()
    y = y64.to(dev) if lik == "classification" else y64.float().to(dev)
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
    loader = _Loader([(X[:4], y[:4]), (X[4:], y[4:])])
    loader.dataset = range(6)
    la = HipLaplace(model, lik, "all", "kron", prior_precision=0.7)
    configure(la.backend)
    la.fit(loader)
    want = None
    for xb, yb in ((X64[:4], y64[:4]), (X64[4:], y64[4:])):
        _, kf = co.kfac_ggn(m64, xb, yb, 6, lik)
        want = kf if want is None else co.kron_add(want, kf)
    for F_, G_ in zip(la.H_facs.kfacs, want):
        for a_, w_ in zip(F_, G_):
            assert rel(a_, w_) < 1e-4, rel(a_, w_)
    swept(la.backend)
    _, f_var = la._glm_predictive_distribution(X)
    Qs, ls = co.kron_decompose(want)
    sig = float(la.sigma_noise)
    assert rel(f_var, functional_variance_kron(Js64, Qs, ls, 0.7, h_factor=1.0 / sig**2)) < 1e-4
    return dict(Js=Js, f=f, h=h, f_var=f_var, kfacs=[t for F_ in la.H_facs.kfacs for t in F_])
