"""Generate tests/golden/tok_{mean,cls}_{classification,regression}.npz by running the UNMODIFIED reference on the models
of tests/embed_fixtures.py (token models: a tracked nn.Embedding and a tracked lone parameter).  Needs the reference sources (oracle/ref_import.py).

TEST INFRASTRUCTURE.  Usage:  ``python -m tools.make_embed_golden``

Per fixture x likelihood, float64 - the subset of oracle/make_golden.py that does not involve KFAC (the reference has no
KFAC rule for embeddings or lone parameters):
  * inputs: model weights / buffers ``w.*``, ``X``, ``y``
  * laplace/curvature/curvature.py: ``Js, f`` (GGNInterface.jacobians :88-129), ``H_ggn, h_ggn, loss`` (:375-433),
    ``H_ef, h_ef, loss_ef`` (EFInterface :467-505)
  * laplace/baselaplace.py through ``Laplace(model, lik, "all", "diag" | "full").fit`` on two minibatches: ``H``, ``loss``,
    GLM ``f_mu, f_var`` (:1306-1342), ``marglik`` (:1074-1109)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402
from tests.embed_fixtures import EMBED_FIXTURES, GOLDEN_DIR, make_fixture  # noqa: E402


#: arrays of at least this many bytes are stored in a file of their own
BIG_BYTES = 256 << 10


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64) if t.is_floating_point() else t.detach().cpu().numpy()


def generate(name: str, likelihood: str) -> dict:
    import_reference()
    from laplace import Laplace
    from laplace.curvature import EFInterface, GGNInterface

    torch.set_default_dtype(torch.float64)
    model, X, y_cls, y_reg = make_fixture(name)
    y = y_cls if likelihood == "classification" else y_reg
    out: dict = {"X": _np(X), "y": _np(y)}
    for k, v in model.state_dict().items():
        out[f"w.{k}"] = _np(v)

    ggn = GGNInterface(model, likelihood)
    Js, f = ggn.jacobians(X)
    loss, H = ggn.full(X, y)
    _, h = ggn.diag(X, y)
    out.update(Js=_np(Js), f=_np(f), H_ggn=_np(H), h_ggn=_np(h), loss=_np(loss))
    ef = EFInterface(model, likelihood)
    loss_ef, H_ef = ef.full(X, y)
    _, h_ef = ef.diag(X, y)
    out.update(H_ef=_np(H_ef), h_ef=_np(h_ef), loss_ef=_np(loss_ef))

    loader = DataLoader(TensorDataset(X, y), batch_size=5)
    sig = SIGMA_NOISE if likelihood == "regression" else 1.0
    for hs in ("diag", "full"):
        tag = f"la.all.{hs}"
        la = Laplace(model, likelihood, subset_of_weights="all", hessian_structure=hs, prior_precision=PRIOR_PREC,
                     sigma_noise=sig, backend=GGNInterface)
        la.fit(loader)
        out[f"{tag}.loss"] = _np(torch.as_tensor(la.loss))
        out[f"{tag}.H"] = _np(la.H)
        f_mu, f_var = la._glm_predictive_distribution(X)
        out[f"{tag}.f_mu"] = _np(f_mu)
        out[f"{tag}.f_var"] = _np(f_var)
        out[f"{tag}.marglik"] = _np(la.log_marginal_likelihood())
    return out


def main():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for name in EMBED_FIXTURES:
        for likelihood in ("classification", "regression"):
            arrays = generate(name, likelihood)
            # dense P x P matrices go into files of their own (`<fixture>_<likelihood>.<key>.npz`): random doubles do not
            # compress, and no file of the repository may exceed 1 MiB; `tests.embed_fixtures.load_golden` merges them
            big = {k: v for k, v in arrays.items() if v.nbytes >= BIG_BYTES}
            paths = [(os.path.join(GOLDEN_DIR, f"{name}_{likelihood}.npz"), {k: v for k, v in arrays.items() if k not in big})]
            paths += [(os.path.join(GOLDEN_DIR, f"{name}_{likelihood}.{k}.npz"), {k: v}) for k, v in big.items()]
            for path, part in paths:
                np.savez_compressed(path, **part)
                size = os.path.getsize(path)
                assert size < (1 << 20), f"{path}: {size} bytes"
                print(f"wrote {path}: {len(part)} arrays, P = {arrays['Js'].shape[-1]}, {size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
