"""The argument contracts of lk_possum_f32, lk_possum_f16x2 and lk_patch_mean_f32 (csrc/lk_kfacreduce.hip), probed at their edges
WITHOUT a device - the method of tests/test_capi_contracts_reduce.py, whose helpers are reused: a table of last-accepted /
first-refused values and a child process that sees no device.  Every check sits in a checker the entry point calls before its
first HIP call; without a device a call that passes ends in LK_ELAUNCH, or in LK_OK when there are no rows (R == 0, B == 0).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, _Probe  # noqa: E402

P32, P16, PM = "lk_possum_f32", "lk_possum_f16x2", "lk_patch_mean_f32"
FAR = [(1 << 61) + (k << 50) for k in range(4)]  # (addresses nothing else is near)
# x: 4 x 8 x 4 floats = 512 bytes at the buffer, y 4096 bytes on
_S = dict(x="same", R=4, L=8, D=4, layout=0, alpha=1.0, y="other")
_H = dict(x_h="same", x_l=FAR[1], sexp=FAR[2], R=4, L=8, D=4, layout=0, alpha=1.0, y="other")
# x: 2 x 4 x 8 x 8 floats = 2048 bytes at the buffer, out 4096 bytes on
_M = dict(x="same", B=2, C=4, H=8, W=8, channels_last=0, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, unfold_order=0, out="other")
_TALL = dict(x=FAR[0], out=FAR[3], B=1, C=1, W=16, channels_last=1, kh=16, kw=16, ph=0, pw=0)  # H * kw floats a channel in LDS


def _shape_rows(fn, base):
    return [
        R(fn, base, {"layout": 1}, {"layout": 2}, f"{fn}: bad arguments (layout is 0"),
        R(fn, base, {"R": 0}, {"R": -1}, f"{fn}: bad arguments (0 <= R"),  # no rows: LK_OK before any HIP call
        R(fn, base, {"L": 1}, {"L": 0}, f"{fn}: bad arguments (0 <= R"),
        R(fn, base, {"D": 1}, {"D": -4}, f"{fn}: bad arguments (0 <= R"),
        R(fn, base, {"y": "other"}, {"y": "same"}, f"{fn}: bad arguments (y overlaps"),
    ]


ROWS = [
    *[R(P32, _S, None, {n: None}, f"{P32}: bad arguments (null pointer)") for n in ("x", "y")],
    R(P32, _S, {"x": FAR[0]}, {"x": FAR[0] + 2}, f"{P32}: bad arguments (x and y are 4-byte aligned)"),
    R(P32, _S, {"y": FAR[0]}, {"y": FAR[0] + 1}, f"{P32}: bad arguments (x and y are 4-byte aligned)"),
    *_shape_rows(P32, _S),
    *[R(P16, _H, None, {n: None}, f"{P16}: bad arguments (null pointer)") for n in ("x_h", "x_l", "sexp", "y")],
    R(P16, _H, {"x_l": FAR[1] + 2}, {"x_l": FAR[1] + 1}, f"{P16}: bad arguments (the planes are 2-byte"),
    R(P16, _H, {"sexp": FAR[2] + 4}, {"sexp": FAR[2] + 2}, f"{P16}: bad arguments (the planes are 2-byte"),
    *_shape_rows(P16, _H),
    R(P16, _H, {"sexp": FAR[2]}, {"sexp": "other"}, f"{P16}: bad arguments (y overlaps"),
    *[R(PM, _M, None, {n: None}, f"{PM}: bad arguments (null pointer)") for n in ("x", "out")],
    R(PM, _M, {"x": FAR[0]}, {"x": FAR[0] + 2}, f"{PM}: bad arguments (x and out are 4-byte aligned)"),
    R(PM, _M, {"channels_last": 1, "unfold_order": 1}, {"channels_last": 2}, f"{PM}: bad arguments (channels_last and"),
    R(PM, _M, {"B": 0}, {"B": -1}, f"{PM}: bad arguments (0 <= B"),  # no samples: LK_OK before any HIP call
    R(PM, _M, {"C": 1}, {"C": 0}, f"{PM}: bad arguments (0 <= B"),
    # a kernel side of 16 on a 16-row map (x then ends where out begins), 17 refused whatever the map
    R(PM, _M, {"kh": 16, "H": 16}, {"kh": 17, "H": 32}, f"{PM}: bad arguments (1 <= kh, kw <= 16)"),
    R(PM, _M, {"kw": 1}, {"kw": 0}, f"{PM}: bad arguments (1 <= kh, kw <= 16)"),
    R(PM, _M, {"sh": 2}, {"sh": 0}, f"{PM}: bad arguments (1 <= stride"),
    R(PM, _M, {"dw": 2}, {"dw": 0}, f"{PM}: bad arguments (1 <= stride"),
    R(PM, _M, {"pw": 0}, {"pw": -1}, f"{PM}: bad arguments (1 <= stride"),
    R(PM, _M, {"H": 1, "ph": 1}, {"H": 1, "ph": 0}, f"{PM}: bad arguments (the dilated kernel is larger"),
    R(PM, _M, {"out": "other"}, {"out": "same"}, f"{PM}: bad arguments (out overlaps x)"),
    # 16 column sums of H rows: 2560 rows fill the 160 KiB of LDS exactly
    R(PM, _M, {**_TALL, "H": 2560}, {**_TALL, "H": 2561}, f"{PM}: bad arguments (the column sums of 1 channels"),
]
SENTINEL = ("lk_symmetrize_f32", {"n": -1})


def _child_main():
    import torch

    def emit(obj):
        sys.stdout.write(json.dumps(obj) + "\n")
        sys.stdout.flush()

    if torch.cuda.device_count() != 0:
        emit({"fatal": "device visible"})
        return 3
    P = _Probe()
    for i, row in enumerate(ROWS):
        for side in ("refuse", "accept"):
            if row[side] is None:
                continue
            emit({"start": [i, side]})
            P.call(*SENTINEL)  # (a refusal of another entry point first: a message of this one can only come from this call)
            rc, msg = P.call(row["fn"], {**row["base"], **row[side]})
            emit({"row": i, "side": side, "rc": rc, "msg": msg})
    emit({"done": True})
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
    rows, last, done = {}, None, False
    for line in proc.stdout.splitlines():
        try:
            obj = json.loads(line)
        except ValueError:
            continue
        if "fatal" in obj:
            pytest.fail(f"the probing child refused to run: {obj['fatal']}")
        last = obj.get("start", last)
        if "row" in obj:
            rows[(obj["row"], obj["side"])] = (obj["rc"], obj["msg"])
        done = done or "done" in obj
    if proc.returncode != 0 or not done:
        pytest.fail(f"the probing child ended with status {proc.returncode}; last probe started: {last}\n" + proc.stderr[-2000:])
    return rows


def _row_id(i):
    return (ROWS[i]["fn"][3:] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items() if k not in _TALL or k == "H"))[:80]


@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_guard_edges(probes, i):
    """first refused -> LK_EINVAL with the guard's own message; last accepted -> anything but a refusal"""
    row = ROWS[i]
    rc, msg = probes[(i, "refuse")]
    assert rc == LK_EINVAL, f"accepted {row['refuse']} (rc={rc}: {msg})"
    assert row["fragment"] in msg, f"refused {row['refuse']} with another message: {msg}"
    if row["accept"] is not None:
        rc, msg = probes[(i, "accept")]
        assert rc in (LK_OK, LK_ELAUNCH), f"refused the in-contract {row['accept']}: rc={rc} {msg}"
        a = {**row["base"], **row["accept"]}
        if a.get("R", a.get("B")) == 0:
            assert rc == LK_OK  # (nothing to do: the call returns before any HIP call)


def test_the_variant_queries_follow_the_entry_points():
    """lk_possum_variant and lk_patch_mean_variant are host code: asked in this process"""
    from laplace_amd._lib import HipKernels

    K = HipKernels()
    assert K.possum_variant(-1, 8, 4) is None and K.possum_variant(4, 0, 4) is None and K.possum_variant(4, 8, 4, layout=2) is None
    # the two regimes: S B = 1152 maps of 32 x 32 x 64 keep 16 lanes across the 16 channel vectors; 128 sequences narrow them
    assert K.possum_variant(1152, 1024, 64) == {"vec": True, "layout": 0, "lanes": 16, "blocks": 1152}
    assert K.possum_variant(128, 64, 192) == {"vec": True, "layout": 0, "lanes": 8, "blocks": 768}
    assert K.possum_variant(128, 64, 192, aligned=False)["vec"] is False
    assert K.possum_variant(1152, 1024, 64, layout=1) == {"vec": True, "layout": 1, "lanes": 64, "blocks": 2048}
    geo = ((3, 3), (1, 1), (1, 1), (1, 1))
    assert K.patch_mean_variant((128, 64, 32, 32), True, *geo) == {"vec": True, "channel_block": 32, "lds_kib": 12}
    assert K.patch_mean_variant((128, 64, 32, 32), False, *geo) == {"vec": True, "channel_block": 32, "lds_kib": 12}
    assert K.patch_mean_variant((1, 1, 2561, 16), True, (16, 16), (1, 1), (0, 0), (1, 1)) is None
    assert K.patch_mean_variant((2, 4, 8, 8), False, (17, 3), (1, 1), (1, 1), (1, 1)) is None
    assert K.patch_mean_variant((2, 4, 8, 8), False, (3, 3), (1, 1), "same", (1, 1)) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
