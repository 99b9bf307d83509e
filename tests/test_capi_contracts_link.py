"""The argument contract of lk_glm_link_f32 and the regimes lk_glm_link_variant names (csrc/lk_link.hip), probed at their edges
WITHOUT a device, after tests/test_capi_contracts_rmsnorm.py: a child process that sees no device calls the library with
addresses nothing ever touches; a refusal is LK_EINVAL with the guard's own message, a call that passes its guards ends in
LK_ELAUNCH.  The helpers of tests/test_capi_contracts.py are reused."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, _Probe  # noqa: E402

FN, VARIANT = "lk_glm_link_f32", "lk_glm_link_variant"
# five regions 16 MiB apart: f_var of 4 samples x 192 x 192 floats is 576 KiB
BASE = dict(f_mu=1 << 24, f_var=2 << 24, z=3 << 24, probs=4 << 24, info=5 << 24, B=4, C=10, n_samples=7, link=1, diag=0)
# (id, last accepted or None, first refused, fragment of the refusal)
EDGES = [
    ("C=0", {"C": 1}, {"C": 0}, "outside 1 <= C <= LK_LINK_MAX_C = 192"),
    ("C=193", {"C": 192}, {"C": 193}, "outside 1 <= C <= LK_LINK_MAX_C = 192"),
    ("link=4", {"link": 3}, {"link": 4}, "link must be 0 (probit), 1 (mc), 2 (bridge) or 3 (bridge_norm)"),
    ("n_samples=0", {"n_samples": 1}, {"n_samples": 0}, "n_samples out of range"),
    ("null-probs", {"z": None, "link": 2}, {"probs": None}, "null pointer"),
    ("null-z-mc", {"z": None, "link": 0}, {"z": None}, "null pointer"),
    ("misaligned", {"z": (3 << 24) + 4, "link": 2}, {"z": (3 << 24) + 4}, "16-byte aligned"),
    # probs [4][10] floats are 160 bytes: right behind f_mu is fine, 16 bytes earlier is not
    ("overlap", {"probs": (1 << 24) + 160}, {"probs": (1 << 24) + 144}, "an output overlaps an input"),
    ("overlap-info", {"info": (4 << 24) + 160}, {"info": (4 << 24) + 144}, "probs overlaps info"),
]
REGIMES = [(64, 0), (65, 1), (192, 1), (193, -1)]


def _child_main():
    import torch

    if torch.cuda.device_count() != 0:
        print(json.dumps({"fatal": "device visible"}))
        return 3
    P = _Probe()
    out = {"edges": {}, "regimes": {}}
    for name, accept, refuse, _ in EDGES:
        P.call("lk_symmetrize_f32", {"n": -1})  # (another entry point's refusal first: a message of this one comes from this call)
        out["edges"][name] = {"refuse": P.call(FN, {**BASE, **refuse}), "accept": P.call(FN, {**BASE, **accept}),
                              "empty": P.call(FN, {**BASE, **accept, "B": 0})}
    for C, _ in REGIMES:
        out["regimes"][str(C)] = [P.call(VARIANT, dict(B=4, C=C, n_samples=7, link=link, diag=0))[0] for link in range(4)]
    print(json.dumps(out))
    return 0


@pytest.fixture(scope="module")
def probes():
    from laplace_amd._lib import LIB_PATH

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child"]
    proc = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, f"the probing child ended with status {proc.returncode}\n{proc.stdout[-500:]}\n{proc.stderr[-2000:]}"
    return json.loads(proc.stdout.splitlines()[-1])


@pytest.mark.parametrize("name,accept,refuse,fragment", EDGES, ids=[e[0] for e in EDGES])
def test_guard_edges(probes, name, accept, refuse, fragment):
    """first refused -> LK_EINVAL with the guard's message; last accepted -> no refusal, and LK_OK for an empty batch"""
    got = probes["edges"][name]
    rc, msg = got["refuse"]
    assert rc == LK_EINVAL and msg.startswith(FN + ": ") and fragment in msg, (rc, msg)
    assert got["accept"][0] in (LK_OK, LK_ELAUNCH), got["accept"]
    assert got["empty"][0] == LK_OK, got["empty"]


@pytest.mark.parametrize("C,regime", REGIMES)
def test_the_variant_names_the_regime(probes, C, regime):
    """a wave per sample up to C = 64, a workgroup per sample up to LK_LINK_MAX_C = 192, refused beyond; the same for every link"""
    got = probes["regimes"][str(C)]
    assert all(r < 0 for r in got) if regime < 0 else got == [regime] * 4, got


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
