"""The argument contract of lk_glm_samples_f32 and what lk_glm_samples_variant names (csrc/lk_glmsamples.hip), probed at their
edges WITHOUT a device, after tests/test_capi_contracts_joint.py: a child process that sees no device calls the library with
addresses nothing ever touches; a refusal is LK_EINVAL with the guard's own message, a call that passes its guards ends in
LK_ELAUNCH."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, _Probe  # noqa: E402

FN, VARIANT = "lk_glm_samples_f32", "lk_glm_samples_variant"
T = 1 << 44
# regions 16 TiB apart (an output of 2^40 floats is 4 TiB); f_mu [4][10] floats are 160 bytes, out [7][4][10] floats 1120 bytes
BASE = dict(f_mu=T, f_var=2 * T, z=3 * T, out=4 * T, info=5 * T, B=4, C=10, n_samples=7, diag=0, softmax=0)
# (id, last accepted, first refused, fragment of the refusal)
EDGES = [
    ("C=0", {"C": 1}, {"C": 0}, "outside 1 <= C <= LK_LINK_MAX_C = 192"),
    ("C=193", {"C": 192}, {"C": 193}, "outside 1 <= C <= LK_LINK_MAX_C = 192"),
    ("diag-C=0", {"C": 1, "diag": 1}, {"C": 0, "diag": 1}, "outside 1 <= C <= LK_LINK_WIDE_MAX_C = 4096"),
    ("diag-C=4097", {"C": 4096, "diag": 1}, {"C": 4097, "diag": 1}, "outside 1 <= C <= LK_LINK_WIDE_MAX_C = 4096"),
    ("n=0", {"n_samples": 1}, {"n_samples": 0}, "n_samples out of range"),
    ("n=2^20", {"n_samples": (1 << 20) - 1}, {"n_samples": 1 << 20}, "n_samples out of range"),
    ("B<0", {"B": 1}, {"B": -1}, "B out of range"),
    ("nBC=2^40", {"B": (1 << 24) - 1, "C": 64, "n_samples": 1 << 10}, {"B": 1 << 24, "C": 64, "n_samples": 1 << 10},
     "n_samples * B * C out of range"),
    ("null-z", {}, {"z": None}, "null pointer"),
    ("null-info", {}, {"info": None}, "null pointer"),
    ("misaligned", {}, {"out": 4 * T + 4}, "16-byte aligned"),
    ("out-overlaps-f_mu", {"out": T + 160}, {"out": T + 144}, "an output overlaps an input"),
    ("f_mu-overlaps-out", {"f_mu": 4 * T + 1120}, {"f_mu": 4 * T + 1104}, "an output overlaps an input"),
    ("info-overlaps-z", {"n_samples": 8, "info": 3 * T + 320}, {"n_samples": 8, "info": 3 * T + 304}, "an output overlaps an input"),
    ("out-overlaps-info", {"info": 4 * T + 1120}, {"info": 4 * T + 1104}, "out overlaps info"),
]
# (B, C, n, diag) -> regime | chunks << 8: the regime boundaries and the chunk rule (stages of 16 draws, 512 workgroups wanted)
VARIANTS = [((128, 64, 100, 0), 0 | 7 << 8), ((128, 65, 100, 0), 1 | 4 << 8), ((128, 192, 100, 0), 1 | 4 << 8),
            ((128, 193, 100, 0), -1), ((128, 4096, 100, 1), 2 | 4 << 8), ((128, 4097, 100, 1), -1), ((5, 10, 40, 0), 0 | 3 << 8),
            ((2048, 2, 17, 0), 0 | 1 << 8), ((512, 17, 33, 1), 2 | 1 << 8), ((1, 1, 1, 0), 0 | 1 << 8), ((4, 10, 0, 0), -1)]


def _child_main():
    import torch

    if torch.cuda.device_count() != 0:
        print(json.dumps({"fatal": "device visible"}))
        return 3
    P = _Probe()
    out = {"edges": {}}
    for name, accept, refuse, _ in EDGES:
        P.call("lk_symmetrize_f32", {"n": -1})  # (another entry point's refusal first: a message of this one comes from this call)
        out["edges"][name] = {"refuse": P.call(FN, {**BASE, **refuse}), "accept": P.call(FN, {**BASE, **accept}),
                              "empty": P.call(FN, {**BASE, **accept, "B": 0})}
    out["variants"] = [P.call(VARIANT, dict(B=B, C=C, n_samples=n, diag=diag, softmax=sm))[0]
                       for (B, C, n, diag), _ in VARIANTS for sm in (0, 1)]
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


def test_the_variant_names_the_regime_and_the_chunks(probes):
    """negative exactly where the entry point refuses the shape; softmax changes neither the regime nor the split"""
    assert probes["variants"] == [v for _, v in VARIANTS for _ in (0, 1)], probes["variants"]


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
