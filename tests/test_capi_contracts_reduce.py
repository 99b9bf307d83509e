"""The argument contracts of lk_maxred_fwd_f32, lk_maxred_vjp_f32 and lk_reduce_variant (csrc/lk_reduce.hip), probed at their edges
WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_slice.py: a
table of last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_reduce.hip keeps every argument check in checker functions that the entry points call before the first HIP call.  Without a
device a call that passes its checker ends in LK_ELAUNCH, or in LK_OK when there are no rows (``outer == 0``).
"""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, _Probe, header_prototypes  # noqa: E402

FWD, VJP = "lk_maxred_fwd_f32", "lk_maxred_vjp_f32"
FAR = [(1 << 61) + (k << 50) for k in range(5)]  # (addresses nothing else is near: no probe of an extent meets the overlap guard)
I30, I31 = (1 << 30) - 1, (1 << 31) - 1

# x: 4 x 8 x 4 floats = 512 bytes at the buffer; y 4096 bytes on; idx and cnt far away
_F = dict(x="same", outer=4, L=8, inner=4, y="other", idx=FAR[1], cnt=FAR[2])
_FARF = dict(x=FAR[0], y=FAR[3])
# g: 2 x 4 x 4 floats = 128 bytes at the buffer; dx 4096 bytes on; the first maximum from idx, far away
_V = dict(g="same", idx=FAR[1], x=None, y=None, cnt=None, S=2, outer=4, L=8, inner=4, dx="other")
_EVEN = dict(idx=None, x=FAR[1], y=FAR[2], cnt=FAR[3])
_FARV = dict(g=FAR[0], dx=FAR[4])
_SHAPE_F = f"{FWD}: bad arguments (0 <= outer"
_SHAPE_V = f"{VJP}: bad arguments (1 <= S"
_MODE = f"{VJP}: bad arguments (give idx alone"
ROWS = [
    # ---- the forward -----------------------------------------------------------------------------------------------------------
    *[R(FWD, _F, None, {name: None}, f"{FWD}: bad arguments (null pointer)") for name in ("x", "y", "idx", "cnt")],
    # 0 <= outer < 2^31; no rows: LK_OK before any HIP call
    R(FWD, _F, {"outer": 0}, {"outer": -1}, _SHAPE_F),
    R(FWD, _F, {"outer": I31, "L": 1, "inner": 1, **_FARF}, {"outer": 1 << 31, "L": 1, "inner": 1, **_FARF}, _SHAPE_F),
    # 1 <= L < 2^30
    R(FWD, _F, {"L": 1}, {"L": 0}, _SHAPE_F),
    R(FWD, _F, {"L": I30, "outer": 1, "inner": 1, **_FARF}, {"L": 1 << 30, "outer": 1, "inner": 1, **_FARF}, _SHAPE_F),
    # 1 <= inner < 2^30
    R(FWD, _F, {"inner": 1}, {"inner": 0}, _SHAPE_F),
    R(FWD, _F, {"inner": I30, "outer": 1, "L": 1, **_FARF}, {"inner": 1 << 30, "outer": 1, "L": 1, **_FARF}, _SHAPE_F),
    # outer * inner < 2^31
    R(FWD, _F, {"outer": 1 << 16, "inner": (1 << 15) - 1, "L": 1, **_FARF}, {"outer": 1 << 16, "inner": 1 << 15, "L": 1, **_FARF}, _SHAPE_F),
    # outer * L * inner < 2^40
    R(FWD, _F, {"outer": (1 << 11) - 1, "L": 1 << 29, "inner": 1, **_FARF}, {"outer": 1 << 11, "L": 1 << 29, "inner": 1, **_FARF}, _SHAPE_F),
    # the outputs overlap neither x nor each other.  x at the buffer (128 bytes a row of outer) and y 4096 bytes on: 32 fit exactly
    R(FWD, _F, {"y": "other"}, {"y": "same"}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, {"outer": 32}, {"outer": 33}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, {"idx": "other", "y": FAR[3]}, {"idx": "same", "y": FAR[3]}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, {"cnt": "other", "y": FAR[3]}, {"cnt": "same", "y": FAR[3]}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, None, {"idx": "other"}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, None, {"cnt": "other"}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    R(FWD, _F, None, {"cnt": FAR[1]}, f"{FWD}: bad arguments (y, idx and cnt overlap"),
    # y (16 bytes a row of outer) at the buffer and x 4096 bytes on: 256 fit exactly
    R(FWD, _F, {"y": "same", "x": "other", "outer": 256}, {"y": "same", "x": "other", "outer": 257},
      f"{FWD}: bad arguments (y, idx and cnt overlap"),
    # ---- the VJP ---------------------------------------------------------------------------------------------------------------
    *[R(VJP, _V, None, {name: None}, f"{VJP}: bad arguments (null pointer)") for name in ("g", "dx")],
    # idx alone, or x, y and cnt (idx is then not looked at)
    R(VJP, _V, {"idx": FAR[1]}, {"idx": None}, _MODE),
    R(VJP, _V, _EVEN, {**_EVEN, "x": None}, _MODE),
    R(VJP, _V, {**_EVEN, "idx": FAR[0]}, {"x": FAR[2]}, _MODE),
    R(VJP, _V, _EVEN, {**_EVEN, "y": None}, _MODE),
    R(VJP, _V, _EVEN, {"cnt": FAR[3]}, _MODE),
    # 1 <= S < 2^31
    R(VJP, _V, {"S": 1}, {"S": 0}, _SHAPE_V),
    R(VJP, _V, {"S": I31, "outer": 1, "L": 1, "inner": 1, **_FARV}, {"S": 1 << 31, "outer": 1, "L": 1, "inner": 1, **_FARV}, _SHAPE_V),
    # the shape, as the forward
    R(VJP, _V, {"outer": 0}, {"outer": -1}, _SHAPE_V),
    R(VJP, _V, {"L": 1}, {"L": 0}, _SHAPE_V),
    R(VJP, _V, {"inner": 1}, {"inner": 0}, _SHAPE_V),
    R(VJP, _V, {"L": I30, "S": 1, "outer": 1, "inner": 1, **_FARV}, {"L": 1 << 30, "S": 1, "outer": 1, "inner": 1, **_FARV}, _SHAPE_V),
    R(VJP, _V, {"inner": I30, "S": 1, "outer": 1, "L": 1, **_FARV}, {"inner": 1 << 30, "S": 1, "outer": 1, "L": 1, **_FARV}, _SHAPE_V),
    R(VJP, _V, {"outer": 1 << 16, "inner": (1 << 15) - 1, "L": 1, "S": 1, **_FARV}, {"outer": 1 << 16, "inner": 1 << 15, "L": 1, "S": 1, **_FARV},
      _SHAPE_V),
    # S * outer * L * inner < 2^40
    R(VJP, _V, {"S": 2, "outer": (1 << 10) - 1, "L": 1 << 29, "inner": 1, **_FARV}, {"S": 2, "outer": 1 << 10, "L": 1 << 29, "inner": 1, **_FARV},
      _SHAPE_V),
    # dx overlaps no operand.  g (32 bytes a row of outer) at the buffer and dx 4096 bytes on: 128 fit exactly
    R(VJP, _V, {"dx": "other"}, {"dx": "same"}, f"{VJP}: bad arguments (dx overlaps"),
    R(VJP, _V, {"outer": 128}, {"outer": 129}, f"{VJP}: bad arguments (dx overlaps"),
    # idx, y, cnt (16 bytes a row of outer): 256; x (128 bytes): 32
    R(VJP, _V, {"g": FAR[0], "idx": "same", "outer": 256}, {"g": FAR[0], "idx": "same", "outer": 257}, f"{VJP}: bad arguments (dx overlaps"),
    R(VJP, _V, {**_EVEN, "g": FAR[0], "x": "same", "outer": 32}, {**_EVEN, "g": FAR[0], "x": "same", "outer": 33}, f"{VJP}: bad arguments (dx overlaps"),
    R(VJP, _V, {**_EVEN, "g": FAR[0], "y": "same", "outer": 256}, {**_EVEN, "g": FAR[0], "y": "same", "outer": 257}, f"{VJP}: bad arguments (dx overlaps"),
    R(VJP, _V, {**_EVEN, "g": FAR[0], "cnt": "same", "outer": 256}, {**_EVEN, "g": FAR[0], "cnt": "same", "outer": 257},
      f"{VJP}: bad arguments (dx overlaps"),
    # (the even split does not look at idx: one that overlaps dx is no refusal)
    R(VJP, _V, {**_EVEN, "idx": "other"}, {"idx": "other"}, f"{VJP}: bad arguments (dx overlaps"),
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
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
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
        elif "start" in obj:
            last = obj["start"]
        elif "row" in obj:
            rows[(obj["row"], obj["side"])] = (obj["rc"], obj["msg"])
        elif "done" in obj:
            done = True
    if proc.returncode != 0 or not done:
        pytest.fail(f"the probing child ended with status {proc.returncode}; last probe started: {last}\n" + proc.stderr[-2000:])
    return rows


def _row_id(i):
    return (ROWS[i]["fn"][10:13] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items()))[:100]


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": bad arguments")
    assert [p[2] for p in protos[FWD]] == ["x", "outer", "L", "inner", "y", "idx", "cnt", "stream"]
    assert [p[2] for p in protos[VJP]] == ["g", "idx", "x", "y", "cnt", "S", "outer", "L", "inner", "dx", "stream"]
    assert [p[2] for p in protos["lk_reduce_variant"]] == ["vjp", "S", "outer", "L", "inner", "even", "aligned"]


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
        if {**row["base"], **row["accept"]}["outer"] == 0:
            assert rc == LK_OK  # (no rows: the call returns before any HIP call)


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_reduce.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for m in re.finditer(r"LK_REQUIRE\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', text[m.end():j])))
    return out


def test_every_guard_of_the_file_is_reached_by_a_row(probes):
    messages = _guard_messages()
    assert len(messages) == 7, messages
    assert all(m.startswith((FWD + ": bad arguments", VJP + ": bad arguments")) for m in messages), messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    missing = [m for m in messages if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_reduce.hip")).read()
    for fn, checker in ((FWD, "maxred_check_fwd("), (VJP, "maxred_check_vjp(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FWD, VJP, "lk_reduce_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_points_refuse():
    """lk_reduce_variant is host code: every numeric row of the table, asked in this process"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if row["fragment"] not in (_SHAPE_F, _SHAPE_V):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            got = K.reduce_variant(row["fn"] == VJP, a.get("S", 1), a["outer"], a["L"], a["inner"], a.get("x") is not None)
            assert (got is not None) == want, (side, row[side], got)
            asked += 1
    assert asked >= 30
    assert K.reduce_variant(True, 9, 128 * 300, 126, 1) == {"vjp": True, "row": True, "vec": False, "even": False, "wide_index": False,
                                                            "lanes": 1, "seed_split": False, "blocks": 2048}
    assert K.reduce_variant(False, 1, 128 * 300, 126, 1)["lanes"] == 64


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
