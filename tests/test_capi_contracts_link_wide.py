"""The argument contract of lk_glm_link_wide_f32, the workspace size lk_glm_link_wide_work_bytes asks for and the kernels
lk_glm_link_wide_variant names (csrc/lk_linkwide.hip), probed at their edges WITHOUT a device, after
tests/test_capi_contracts_link.py: a child process that sees no device calls the library with addresses nothing ever touches; a
refusal is LK_EINVAL with the guard's own message, a call that passes its guards ends in LK_ELAUNCH."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, _Probe  # noqa: E402

FN, VARIANT, WORK = "lk_glm_link_wide_f32", "lk_glm_link_wide_variant", "lk_glm_link_wide_work_bytes"
SLAB193 = 224 * 224 * 4  # CP = 32 ceil(193 / 32) = 224
# regions 1 GiB apart: f_var of 2 samples x 4096 x 4096 floats is 128 MiB; the workspace is the last one
BASE = dict(f_mu=1 << 30, f_var=2 << 30, z=3 << 30, probs=4 << 30, info=5 << 30, work=6 << 30, work_bytes=1 << 30, B=2, C=193,
            n_samples=7, link=1, diag=0)
# (id, last accepted, first refused, fragment of the refusal)
EDGES = [
    ("C=192", {"C": 193}, {"C": 192}, "lk_glm_link_f32 serves that range"),
    ("C=4097-probit", {"C": 4096, "link": 0}, {"C": 4097, "link": 0}, "above LK_LINK_WIDE_MAX_C = 4096"),
    ("C=4097-bridge", {"C": 4096, "link": 2}, {"C": 4097, "link": 2}, "above LK_LINK_WIDE_MAX_C = 4096"),
    ("C=4097-mc-diag", {"C": 4096, "diag": 1}, {"C": 4097, "diag": 1}, "above LK_LINK_WIDE_MAX_C = 4096"),
    ("C=225-mc-full", {"C": 224}, {"C": 225}, "above LK_LINK_WIDE_MAX_C_FULL = 224"),
    ("work-one-slab", {"work_bytes": SLAB193}, {"work_bytes": SLAB193 - 4}, "holds no slab"),
    ("null-work", {"work": None, "diag": 1}, {"work": None}, "null workspace"),
    ("misaligned-work", {"work": (6 << 30) + 4, "link": 2}, {"work": (6 << 30) + 4}, "workspace must be 16-byte aligned"),
    # probs [2][193] floats are 1544 bytes; two slabs are used (B = 2)
    ("work-overlap", {"work": (4 << 30) + 1552}, {"work": (4 << 30) + 1536}, "the workspace overlaps an output"),
    ("n_samples=0", {"n_samples": 1}, {"n_samples": 0}, "n_samples out of range"),
    ("link=4", {"link": 3}, {"link": 4}, "link must be 0 (probit), 1 (mc), 2 (bridge) or 3 (bridge_norm)"),
]
# (C, link, diag) -> the kernel; the four regimes and their limits
VARIANTS = [((193, 0, 0), 0), ((4096, 2, 0), 0), ((4096, 3, 1), 0), ((193, 1, 1), 1), ((4096, 1, 1), 1), ((193, 1, 0), 2),
            ((224, 1, 0), 2), ((225, 1, 0), -1), ((192, 1, 0), -1), ((4097, 0, 0), -1)]
# (B, C, link, diag) -> bytes: min(B, 256) slabs for mc with the full covariance, nothing otherwise
WORK_BYTES = [((1, 200, 1, 0), SLAB193), ((256, 193, 1, 0), 256 * SLAB193), ((1000, 193, 1, 0), 256 * SLAB193),
              ((1000, 193, 1, 1), 0), ((1000, 193, 0, 0), 0), ((4, 225, 1, 0), 0)]


def _child_main():
    import ctypes

    import torch

    if torch.cuda.device_count() != 0:
        print(json.dumps({"fatal": "device visible"}))
        return 3
    P = _Probe()
    getattr(P.lib, WORK).restype = ctypes.c_int64
    out = {"edges": {}}
    for name, accept, refuse, _ in EDGES:
        P.call("lk_symmetrize_f32", {"n": -1})  # (another entry point's refusal first: a message of this one comes from this call)
        out["edges"][name] = {"refuse": P.call(FN, {**BASE, **refuse}), "accept": P.call(FN, {**BASE, **accept}),
                              "empty": P.call(FN, {**BASE, **accept, "B": 0})}
    out["variants"] = [P.call(VARIANT, dict(B=4, C=C, n_samples=7, link=link, diag=diag))[0] for (C, link, diag), _ in VARIANTS]
    out["work"] = [P.call(WORK, dict(B=B, C=C, link=link, diag=diag))[0] for (B, C, link, diag), _ in WORK_BYTES]
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


def test_the_variant_names_the_kernel(probes):
    want = [v for _, v in VARIANTS]
    assert [(-1 if g < 0 else g) for g in probes["variants"]] == want, probes["variants"]


def test_the_workspace_size(probes):
    assert probes["work"] == [v for _, v in WORK_BYTES], probes["work"]


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
