"""The argument contract of lk_nn_head_f32, the workspace it asks for and the shapes lk_nn_head_variant refuses
(csrc/lk_nnhead.hip), probed at their edges WITHOUT a device, after tests/test_capi_contracts_link.py: a child process that sees no
device calls the library with addresses nothing ever touches; a refusal comes with the guard's own message, a call that passes its
guards ends in LK_ELAUNCH."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, _Probe  # noqa: E402

FN, VARIANT, LK_EWORKSPACE = "lk_nn_head_f32", "lk_nn_head_variant", -2
# regions 1 GiB apart; P = 10 * 8 + 10 = 90; seven draw groups of [4][10] floats: 1120 bytes of workspace
BASE = dict(phi=1 << 30, theta=2 << 30, out=3 << 30, out2=4 << 30, work=5 << 30, work_bytes=1 << 30, B=4, C=10, D=8, S=7, ld=90,
            has_bias=1, mode=0, softmax=0)
# (id, last accepted, first refused, code and fragment of the refusal)
EDGES = [
    ("C=0", {"C": 1}, {"C": 0}, LK_EINVAL, "outside 1 <= C <= LK_NN_HEAD_MAX_C = 1024"),
    ("C=1025", {"C": 1024, "ld": 1024 * 9}, {"C": 1025, "ld": 1025 * 9}, LK_EINVAL, "outside 1 <= C <= LK_NN_HEAD_MAX_C = 1024"),
    ("S=0", {"S": 1}, {"S": 0}, LK_EINVAL, "S out of range"),
    ("ld<P", {"ld": 90}, {"ld": 89}, LK_EINVAL, "below the 90 parameters"),
    ("null-out", {"out2": None}, {"out": None}, LK_EINVAL, "null pointer"),
    ("null-var", {"out2": None, "mode": 2}, {"out2": None, "mode": 1}, LK_EINVAL, "null pointer"),
    ("misaligned", {"out2": (4 << 30) + 4}, {"out2": (4 << 30) + 4, "mode": 1}, LK_EINVAL, "16-byte aligned"),
    # phi [4][8] floats are 128 bytes: right behind it is fine, 16 bytes earlier is not
    ("overlap", {"out": (1 << 30) + 128}, {"out": (1 << 30) + 112}, LK_EINVAL, "an output overlaps an input"),
    ("null-work", {"work": None, "S": 1}, {"work": None}, LK_EINVAL, "null workspace"),
    ("work-overlap", {"work": (3 << 30) + 160}, {"work": (3 << 30) + 144}, LK_EINVAL, "the workspace overlaps an output"),
    ("work-bytes", {"work_bytes": 1120}, {"work_bytes": 1119}, LK_EWORKSPACE, "1120 needed"),
    ("mode=3", {"mode": 2}, {"mode": 3}, LK_EINVAL, "mode must be 0 (probs), 1 (moments) or 2 (samples)"),
]
# (B, C, D, S, mode): the variant is negative exactly where the entry point refuses the shape
SHAPES = [(4, 1, 8, 7, 0), (4, 1024, 8, 7, 2), (4, 64, 1, 1, 1), (4, 0, 8, 7, 0), (4, 1025, 8, 7, 0), (4, 10, 0, 7, 0), (4, 10, 8, 0, 1),
          (4, 10, 8, 1 << 20, 0), (-1, 10, 8, 7, 0), (4, 10, 8, 7, 3), (4, 10, 8, 7, -1)]


def _child_main():
    import torch

    if torch.cuda.device_count() != 0:
        print(json.dumps({"fatal": "device visible"}))
        return 3
    P = _Probe()
    out = {"edges": {}}
    for name, accept, refuse, _, _ in EDGES:
        P.call("lk_symmetrize_f32", {"n": -1})  # (another entry point's refusal first: a message of this one comes from this call)
        out["edges"][name] = {"refuse": P.call(FN, {**BASE, **refuse}), "accept": P.call(FN, {**BASE, **accept}),
                              "empty": P.call(FN, {**BASE, **accept, "B": 0})}
    out["shapes"] = [(P.call(VARIANT, dict(B=B, C=C, D=D, S=S, mode=m))[0],
                      P.call(FN, {**BASE, "B": B, "C": C, "D": D, "S": S, "mode": m, "ld": max(C * D + C, 1)})[0])
                     for B, C, D, S, m in SHAPES]
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


@pytest.mark.parametrize("name,accept,refuse,code,fragment", EDGES, ids=[e[0] for e in EDGES])
def test_guard_edges(probes, name, accept, refuse, code, fragment):
    """first refused -> the code with the guard's message; last accepted -> no refusal, and LK_OK for an empty batch"""
    got = probes["edges"][name]
    rc, msg = got["refuse"]
    assert rc == code and msg.startswith(FN + ": ") and fragment in msg, (rc, msg)
    assert got["accept"][0] in (LK_OK, LK_ELAUNCH), got["accept"]
    assert got["empty"][0] == LK_OK, got["empty"]


def test_the_variant_is_negative_where_the_entry_point_refuses(probes):
    got = [(v < 0, rc == LK_EINVAL) for v, rc in probes["shapes"]]
    assert got == [(i >= 3, i >= 3) for i in range(len(SHAPES))], probes["shapes"]


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
