"""The argument contract of lk_kron_joint_linear_f32 / lk_diag_joint_linear_f32, the workspace they ask for and the shapes
lk_joint_linear_variant refuses (csrc/lk_joint.hip), probed at their edges WITHOUT a device, after
tests/test_capi_contracts_nn_head.py: a child process that sees no device calls the library with addresses nothing ever touches; a
refusal comes with the guard's own message, a call that passes its guards ends in LK_ELAUNCH."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, _Probe  # noqa: E402

KRON, DIAG, VARIANT, LK_EWORKSPACE = "lk_kron_joint_linear_f32", "lk_diag_joint_linear_f32", "lk_joint_linear_variant", -2
G = 1 << 30
# regions 1 GiB apart; one pair block and three Do tiles, one per workgroup: [3][1][256][2][2][2] floats = 24576 bytes of workspace;
# u is [2][4][65] floats = 2080 bytes, cov [8][8] floats = 256 bytes
BASE = {KRON: dict(u=G, v=2 * G, l1=3 * G, l2=4 * G, delta=5 * G, ub=6 * G, lb=7 * G, delta_b=8 * G, cov=9 * G, ws=10 * G,
                   ws_bytes=1 << 20, B=4, C=2, Do=65, Di=8),
        DIAG: dict(a=G, g=2 * G, var_w=3 * G, var_b=4 * G, cov=9 * G, ws=10 * G, ws_bytes=1 << 20, B=4, C=2, Do=65, Di=8)}
# B C = 2^31 - 2 rows: every operand far from the others (cov alone spans 2^64 bytes)
HUGE = dict(Do=1, Di=1, C=2, u=1 << 40, v=2 << 40, l1=3 << 40, l2=(3 << 40) + 64, delta=(3 << 40) + 128, ub=None, lb=None,
            delta_b=None, cov=1 << 50, ws=None)
# (id, entry point, last accepted, first refused, code and fragment of the refusal)
EDGES = [
    ("C=0", KRON, {"C": 1}, {"C": 0}, LK_EINVAL, "outside 1 <= C <= LK_JOINT_MAX_C = 4"),
    ("C=5", KRON, {"C": 4}, {"C": 5}, LK_EINVAL, "outside 1 <= C <= LK_JOINT_MAX_C = 4"),
    ("diag-C=5", DIAG, {"C": 4}, {"C": 5}, LK_EINVAL, "outside 1 <= C <= LK_JOINT_MAX_C = 4"),
    ("null-u", KRON, {}, {"u": None}, LK_EINVAL, "null pointer"),
    ("null-delta", KRON, {}, {"delta": None}, LK_EINVAL, "null pointer"),
    ("null-cov", KRON, {}, {"cov": None}, LK_EINVAL, "null pointer"),
    ("diag-null-var_w", DIAG, {"var_b": None}, {"var_w": None}, LK_EINVAL, "null pointer"),
    ("ub-without-lb", KRON, {"ub": None, "lb": None, "delta_b": None}, {"lb": None}, LK_EINVAL, "bias block needs lb"),
    ("ub-without-delta_b", KRON, {"ub": None, "delta_b": None}, {"delta_b": None}, LK_EINVAL, "bias block needs lb"),
    ("null-ws", KRON, {"ws": None, "Do": 32}, {"ws": None}, LK_EWORKSPACE, "24576 needed"),
    ("ws-bytes", KRON, {"ws_bytes": 24576}, {"ws_bytes": 24575}, LK_EWORKSPACE, "24576 needed"),
    ("ws-overlaps-cov", KRON, {"ws": 9 * G + 256}, {"ws": 9 * G + 252}, LK_EINVAL, "the workspace overlaps cov"),
    ("ws-overlaps-input", DIAG, {"ws": 2 * G + 2080}, {"ws": 2 * G + 2076}, LK_EINVAL, "the workspace overlaps an input"),
    ("cov-overlaps-u", KRON, {"cov": G + 2080}, {"cov": G + 2076}, LK_EINVAL, "cov overlaps an input"),
    ("B*C=2^31", KRON, {**HUGE, "B": (1 << 30) - 1}, {**HUGE, "B": 1 << 30}, LK_EINVAL, "B * C out of range"),
    ("B<0", KRON, {"B": 1}, {"B": -1}, LK_EINVAL, "B * C out of range"),
    ("Do=0", KRON, {"Do": 1}, {"Do": 0}, LK_EINVAL, "Do, Di out of range"),
]
# (mode, B, C, Do, Di): the variant is negative exactly where the entry points refuse the shape (mode 2 has no entry point)
SHAPES = [(0, 4, 1, 8, 8), (1, 4, 4, 65, 8), (0, 0, 2, 8, 8), (1, 1, 3, 1, 1), (0, 4, 0, 8, 8), (1, 4, 5, 8, 8), (0, 1 << 30, 2, 1, 1),
          (0, -1, 2, 8, 8), (1, 4, 2, 0, 8), (0, 4, 2, 8, (1 << 30) + 1), (2, 4, 2, 8, 8), (-1, 4, 2, 8, 8)]
N_ACCEPTED = 4


def _child_main():
    import torch

    if torch.cuda.device_count() != 0:
        print(json.dumps({"fatal": "device visible"}))
        return 3
    P = _Probe()
    out = {"edges": {}}
    for name, fn, accept, refuse, _, _ in EDGES:
        P.call("lk_symmetrize_f32", {"n": -1})  # (another entry point's refusal first: a message of this one comes from this call)
        out["edges"][name] = {"refuse": P.call(fn, {**BASE[fn], **refuse}), "accept": P.call(fn, {**BASE[fn], **accept}),
                              "empty": P.call(fn, {**BASE[fn], **accept, "B": 0})}
    out["shapes"] = []
    for mode, B, C, Do, Di in SHAPES:
        fn = {0: KRON, 1: DIAG}.get(mode)
        far = dict(HUGE, u=1 << 40) if fn == KRON else dict(a=1 << 40, g=2 << 40, var_w=3 << 40, var_b=None, cov=1 << 50)
        rc = P.call(fn, {**BASE[fn], **far, "B": B, "C": C, "Do": Do, "Di": Di, "ws": 1 << 45, "ws_bytes": 1 << 40})[0] if fn else LK_EINVAL
        out["shapes"].append((P.call(VARIANT, dict(mode=mode, B=B, C=C, Do=Do, Di=Di))[0], rc))
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


@pytest.mark.parametrize("name,fn,accept,refuse,code,fragment", EDGES, ids=[e[0] for e in EDGES])
def test_guard_edges(probes, name, fn, accept, refuse, code, fragment):
    """first refused -> the code with the guard's message; last accepted -> no refusal, and LK_OK for an empty batch"""
    got = probes["edges"][name]
    rc, msg = got["refuse"]
    assert rc == code and msg.startswith(fn + ": ") and fragment in msg, (rc, msg)
    assert got["accept"][0] in (LK_OK, LK_ELAUNCH), got["accept"]
    assert got["empty"][0] == LK_OK, got["empty"]


def test_the_variant_is_negative_where_the_entry_points_refuse(probes):
    got = [(v < 0, rc == LK_EINVAL) for v, rc in probes["shapes"]]
    assert got == [(i >= N_ACCEPTED, i >= N_ACCEPTED) for i in range(len(SHAPES))], probes["shapes"]


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
