"""The argument contracts of lk_gate_reduce_nhwc_f32, lk_gate_vjp_nhwc_f32 and lk_gate_variant (csrc/lk_gate.hip), probed at their
edges WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_mul.py:
a table of last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_gate.hip keeps every argument check in checker functions (``gate_check*``) that the entry points call before the first HIP call
(the guards on the two forms of the cotangent and on the extents are functions of their own, shared by both entry points and - the
extents - by lk_gate_variant, and report under their caller's name).  Without a device a call that passes its checker ends in
LK_ELAUNCH, or in LK_OK when there are no samples.

Pointers: "same" is the probe's buffer, "other" 4096 bytes on; an integer is an address as it stands.
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

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, header_prototypes, _Probe  # noqa: E402

RED, VJP = "lk_gate_reduce_nhwc_f32", "lk_gate_vjp_nhwc_f32"
# buffers far from each other and from the probe's own: no probe of an extent meets the overlap guard
G, GH, GL, SX, X, DS, GT, RR, DX, AM = ((1 << 62) + (i << 56) for i in range(10))
I30 = (1 << 30) - 1
# g [2 * 4][16][8] as an fp32 map; x [4][16][8], ds [2 * 4][8]; gate [4][8], r [2 * 4][8], dx [2 * 4][16][8]
_F = dict(g=G, g_h=None, g_l=None, sexp=None, S=2, B=4, P=16, C=8)
_S = dict(g=None, g_h=GH, g_l=GL, sexp=SX, S=2, B=4, P=16, C=8)  # the same as a split tensor
BASE = {RED: dict(x=X, ds=DS), VJP: dict(gate=GT, r=RR, dx=DX, amax=AM)}
OUT = {RED: "ds", VJP: "dx"}
OVERLAP = {RED: f"{RED}: ds overlaps an input", VJP: f"{VJP}: dx overlaps an input or the amax word"}


def _shared(fn):
    f, s = {**_F, **BASE[fn]}, {**_S, **BASE[fn]}
    ext, big = f"{fn}: extent out of range (1 <= S", f"{fn}: extent out of range (S * B * P * C"
    return [
        # the two forms of g: exactly one
        R(fn, f, None, {"g": None}, f"{fn}: null pointer (g: "),
        R(fn, f, {"g": None, "g_h": GH, "g_l": GL, "sexp": SX}, {"g_h": GH}, f"{fn}: both forms of g given"),
        R(fn, f, None, {"g_l": GL}, f"{fn}: both forms of g given"),
        R(fn, f, None, {"sexp": SX}, f"{fn}: both forms of g given"),
        *[R(fn, s, None, {name: None}, f"{fn}: null pointer (the split form of g needs") for name in ("g_h", "g_l", "sexp")],
        # 1 <= S; 0 <= B (no samples: LK_OK before any HIP call); 1 <= P, C < 2^30
        R(fn, f, {"S": 1}, {"S": 0}, ext),
        R(fn, f, {"B": 0}, {"B": -1}, ext),
        R(fn, s, {"B": 0}, {"B": -1}, ext),
        R(fn, f, {"P": 1}, {"P": 0}, ext),
        R(fn, f, {"C": 1}, {"C": 0}, ext),
        R(fn, f, {"P": I30, "S": 1, "B": 1, "C": 1}, {"P": 1 << 30, "S": 1, "B": 1, "C": 1}, ext),
        R(fn, f, {"C": I30, "S": 1, "B": 1, "P": 1}, {"C": 1 << 30, "S": 1, "B": 1, "P": 1}, ext),
        # S * B * P * C < 2^40, approached along each factor
        *[R(fn, f, {**dict(S=1 << 10, B=1 << 10, P=1 << 10, C=1 << 10), k: (1 << 10) - 1}, dict(S=1 << 10, B=1 << 10, P=1 << 10, C=1 << 10), big)
          for k in ("S", "B", "P", "C")],
        R(fn, s, {"S": (1 << 40) - 1, "B": 1, "P": 1, "C": 1}, {"S": 1 << 40, "B": 1, "P": 1, "C": 1}, big),
        # the output must not overlap g in either form: g (2 B 16 8 floats / halves) at the buffer, the output 4096 bytes on
        R(fn, {**f, "g": "same", OUT[fn]: "other"}, {"B": 4}, {"B": 5}, OVERLAP[fn]),
        R(fn, {**s, "g_h": "same", OUT[fn]: "other"}, {"B": 8}, {"B": 9}, OVERLAP[fn]),
        R(fn, {**s, "g_l": "same", OUT[fn]: "other"}, {"B": 8}, {"B": 9}, OVERLAP[fn]),
        R(fn, {**f, "g": "same"}, {OUT[fn]: "other"}, {OUT[fn]: "same"}, OVERLAP[fn]),
    ]


ROWS = [
    *_shared(RED),
    *[R(RED, {**_F, **BASE[RED]}, None, {name: None}, f"{RED}: null pointer (x, ds)") for name in ("x", "ds")],
    # ds (2 B 8 floats) at the buffer: g, a plane or the scale word 4096 bytes on - 64 samples fit exactly; x (B 16 8 floats) at the buffer
    R(RED, {**_F, **BASE[RED], "ds": "same", "g": "other"}, {"B": 64}, {"B": 65}, OVERLAP[RED]),
    R(RED, {**_S, **BASE[RED], "ds": "same", "g_l": "other"}, {"B": 64}, {"B": 65}, OVERLAP[RED]),
    R(RED, {**_S, **BASE[RED], "ds": "same", "sexp": "other"}, {"B": 64}, {"B": 65}, OVERLAP[RED]),
    R(RED, {**_F, **BASE[RED], "x": "same", "ds": "other"}, {"B": 8}, {"B": 9}, OVERLAP[RED]),
    R(RED, {**_F, **BASE[RED], "ds": "same", "x": "other"}, {"B": 64}, {"B": 65}, OVERLAP[RED]),
    *_shared(VJP),
    *[R(VJP, {**_F, **BASE[VJP]}, None, {name: None}, f"{VJP}: null pointer (gate, dx)") for name in ("gate", "dx")],
    # r and the amax word are optional
    R(VJP, {**_F, **BASE[VJP]}, {"r": None}, {"r": None, "gate": None}, f"{VJP}: null pointer (gate, dx)"),
    R(VJP, {**_S, **BASE[VJP]}, {"amax": None, "r": None}, {"amax": None, "dx": None}, f"{VJP}: null pointer (gate, dx)"),
    # dx (2 B 16 8 floats) at the buffer: g, gate, r or the amax word 4096 bytes on - four samples fit exactly
    *[R(VJP, {**_F, **BASE[VJP], "dx": "same", name: "other"}, {"B": 4}, {"B": 5}, OVERLAP[VJP]) for name in ("g", "gate", "r", "amax")],
    # gate (B 8 floats) and r (2 B 8 floats) at the buffer, dx 4096 bytes on
    R(VJP, {**_F, **BASE[VJP], "gate": "same", "dx": "other"}, {"B": 128}, {"B": 129}, OVERLAP[VJP]),
    R(VJP, {**_F, **BASE[VJP], "r": "same", "dx": "other"}, {"B": 64}, {"B": 65}, OVERLAP[VJP]),
    # without r, its address is not looked at
    R(VJP, {**_F, **BASE[VJP], "gate": "same", "dx": "other", "r": None}, {"B": 128}, {"B": 129}, OVERLAP[VJP]),
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
    return ROWS[i]["fn"][8:14] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items())[:70] + f"#{i}"


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")
    assert [p[2] for p in protos[RED]] == ["g", "g_h", "g_l", "sexp", "x", "S", "B", "P", "C", "ds", "stream"]
    assert [p[2] for p in protos[VJP]] == ["g", "g_h", "g_l", "sexp", "gate", "r", "S", "B", "P", "C", "dx", "amax", "stream"]
    assert [p[2] for p in protos["lk_gate_variant"]] == ["vjp", "S", "B", "P", "C", "aligned"]


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
        if {**row["base"], **row["accept"]}["B"] == 0:
            assert rc == LK_OK  # (no samples: the call returns before any HIP call)


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_gate.hip")).read()
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
    """every LK_REQUIRE of lk_gate.hip: a row's first-refused call came back with that guard's message (the guards of the shared
    checkers - their literal starts with "%s: " - under the name of EACH of the two entry points)"""
    messages = _guard_messages()
    assert len(messages) == 9, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = [fn + m[2:] for m in messages if m.startswith("%s: ") for fn in (RED, VJP)] + [m for m in messages if not m.startswith("%s: ")]
    assert len(want) == 5 * 2 + 4 and all(m.startswith((RED + ": ", VJP + ": ")) for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_gate.hip")).read()
    for fn, checker in ((RED, "gate_check_reduce("), (VJP, "gate_check_vjp(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("if (B == 0) return LK_OK") < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {RED, VJP, "lk_gate_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_is_negative_exactly_where_the_entry_points_refuse():
    """lk_gate_variant is host code: every extent row of the table, asked in this process - a dict on the accepted side, None on the
    refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if "extent out of range" not in row["fragment"]:
            continue
        for side, want in (("accept", True), ("refuse", False)):
            a = {**row["base"], **row[side]}
            got = K.gate_variant(row["fn"] == VJP, a["S"], a["B"], a["P"], a["C"])
            assert (got is not None) == want, (side, row[side], got)
            asked += 1
    assert asked == 2 * 2 * 12
    lib = K.lib
    assert lib.lk_gate_variant(2, 2, 4, 16, 8, 1) == -1 and lib.lk_gate_variant(-1, 2, 4, 16, 8, 1) == -1
    assert lib.lk_gate_variant(0, 2, 4, 16, 8, 1) >= 0 and lib.lk_gate_variant(1, 2, 4, 16, 8, 0) >= 0


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
