"""The argument contracts of lk_resample_vjp_f32 and lk_resample_variant (csrc/lk_resample.hip), probed at their edges WITHOUT a
device - the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_reduce.py: a table of
last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_resample.hip keeps every argument check in a checker function that the entry point calls before the first HIP call; without a
device a call that passes it ends in LK_ELAUNCH.  The tap tables live on the device and are not looked into by the entry point
(the wrapper validates them when it packs them: tests/test_resample_fixtures.py); the tap COUNT has its edge in lk_resample_variant,
which is host code."""
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

VJP = "lk_resample_vjp_f32"
FAR = [(1 << 61) + (k << 50) for k in range(8)]  # (addresses nothing else is near: no probe of an extent meets the overlap guard)
I30 = (1 << 30) - 1
TABLES = dict(ptr_h=FAR[1], idx_h=FAR[2], w_h=FAR[3], ptr_w=FAR[4], idx_w=FAR[5], w_w=FAR[6])
# g: 2 x 4 x 8 floats = 256 bytes at the buffer; dx (2 x 2 x 4 floats = 64 bytes) 4096 bytes on; the tables far away
_V = dict(g="same", P=2, OH=4, OW=8, H=2, W=4, dx="other", **TABLES)
_FARV = dict(g=FAR[0], dx=FAR[7])
_SHAPE = f"{VJP}: bad arguments (1 <= P"
_OVER = f"{VJP}: bad arguments (dx overlaps"
ROWS = [
    *[R(VJP, _V, None, {name: None}, f"{VJP}: bad arguments (null pointer)") for name in ("g", "dx", *TABLES)],
    # 1 <= P
    R(VJP, _V, {"P": 1}, {"P": 0}, _SHAPE),
    R(VJP, _V, None, {"P": -1}, _SHAPE),
    # 1 <= OH, OW, H, W < 2^30
    *[R(VJP, _V, {n: 1}, {n: 0}, _SHAPE) for n in ("OH", "OW", "H", "W")],
    *[R(VJP, _V, {"P": 1, "OH": 1, "OW": 1, "H": 1, "W": 1, n: I30, **_FARV}, {"P": 1, "OH": 1, "OW": 1, "H": 1, "W": 1, n: 1 << 30, **_FARV}, _SHAPE)
      for n in ("OH", "OW", "H", "W")],
    # P * max(OH * OW, H * W) < 2^40, on either side
    R(VJP, _V, {"P": (1 << 20) - 1, "OH": 1 << 10, "OW": 1 << 10, "H": 1, "W": 1, **_FARV},
      {"P": 1 << 20, "OH": 1 << 10, "OW": 1 << 10, "H": 1, "W": 1, **_FARV}, _SHAPE),
    R(VJP, _V, {"P": (1 << 20) - 1, "OH": 1, "OW": 1, "H": 1 << 10, "W": 1 << 10, **_FARV},
      {"P": 1 << 20, "OH": 1, "OW": 1, "H": 1 << 10, "W": 1 << 10, **_FARV}, _SHAPE),
    R(VJP, _V, {"P": (1 << 40) - 1, "OH": 1, "OW": 1, "H": 1, "W": 1, **_FARV}, {"P": 1 << 40, "OH": 1, "OW": 1, "H": 1, "W": 1, **_FARV}, _SHAPE),
    # dx overlaps no operand.  g (128 bytes a plane) at the buffer and dx 4096 bytes on: 32 planes fit exactly
    R(VJP, _V, {"dx": "other"}, {"dx": "same"}, _OVER),
    R(VJP, _V, {"P": 32}, {"P": 33}, _OVER),
    # dx (32 bytes a plane) at the buffer and g 4096 bytes on: 128 planes fit exactly
    R(VJP, _V, {"dx": "same", "g": "other", "P": 128}, {"dx": "same", "g": "other", "P": 129}, _OVER),
    # the ptr arrays in full (ptr_h: H + 1 = 3 ints at the buffer + 4096; dx reaches it from the 128th plane on), the tap arrays
    # by their first entry
    R(VJP, _V, {"dx": "same", "g": FAR[0], "ptr_h": "other", "P": 128}, {"dx": "same", "g": FAR[0], "ptr_h": "other", "P": 129}, _OVER),
    R(VJP, _V, {"dx": "same", "g": FAR[0], "ptr_w": "other", "P": 128}, {"dx": "same", "g": FAR[0], "ptr_w": "other", "P": 129}, _OVER),
    *[R(VJP, _V, {"dx": "same", "g": FAR[0], n: "other", "P": 128}, {"dx": "same", "g": FAR[0], n: "other", "P": 129}, _OVER)
      for n in ("idx_h", "w_h", "idx_w", "w_w")],
    R(VJP, _V, None, {"g": FAR[0], "ptr_h": "other", "dx": "other"}, _OVER),
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
    return ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items())[:100]


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": bad arguments")
    assert [p[2] for p in protos[VJP]] == ["g", "P", "OH", "OW", "H", "W", "ptr_h", "idx_h", "w_h", "ptr_w", "idx_w", "w_w", "dx", "stream"]
    assert [p[2] for p in protos["lk_resample_variant"]] == ["P", "OH", "OW", "H", "W", "taps_h", "taps_w", "aligned"]


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


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_resample.hip")).read()
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
    assert len(messages) == 3, messages
    assert all(m.startswith(VJP + ": bad arguments") for m in messages), messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    missing = [m for m in messages if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_point_checks_through_its_checker_only():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_resample.hip")).read()
    body = text[text.index(f'extern "C" int {VJP}'):]
    body = body[:body.index("\n}\n")]
    assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
    assert body.index("resample_check_vjp(") < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {VJP, "lk_resample_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_point_refuses_and_holds_the_tap_cap():
    """lk_resample_variant is host code: every numeric row of the table, asked in this process; the last accepted and the first
    refused tap count of each axis"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if row["fragment"] != _SHAPE:
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            got = K.resample_variant(a["P"], a["OH"], a["OW"], a["H"], a["W"], 1, 1)
            assert (got is not None) == want, (side, row[side], got)
            asked += 1
    assert asked >= 20
    cap = K.RESAMPLE_MAX_TAPS
    header = open(os.path.join(ROOT, "include", "laplace_hip.h")).read()
    assert cap == int(re.search(r"#define LK_RESAMPLE_MAX_TAPS (\d+)", header).group(1)) >= 16
    for th, tw, want in ((cap, cap, True), (cap + 1, 1, False), (1, cap + 1, False), (0, 0, True), (-1, 1, False), (1, -1, False)):
        assert (K.resample_variant(2, 4, 8, 2, 4, th, tw) is not None) == want, (th, tw)
    assert K.resample_variant(2, 4, 8, 2, 4, 4, 4)["taps_in_registers"] and not K.resample_variant(2, 4, 8, 2, 4, 5, 1)["taps_in_registers"]
    assert K.resample_variant(576, 64, 64, 32, 32, 2, 2) == {"vec": True, "taps_in_registers": True, "wide_index": False, "plane_split": True,
                                                             "grid_stride": False, "packed_slices": False, "blocks": 1}
    assert K.resample_variant(576, 64, 64, 32, 32, 2, 2, aligned=False)["blocks"] == 4
    assert K.resample_variant(54, 4, 4, 2, 2, 2, 2, aligned=False)["packed_slices"]  # (4 lanes a plane: 64 slices a workgroup)


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
