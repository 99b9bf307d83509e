"""The argument contracts of lk_mul_vjp_f32 and lk_mul_variant (csrc/lk_mul.hip), probed at their edges WITHOUT a device - the method
of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_slice.py: a table of last-accepted /
first-refused values, a child process that sees no device, and a completeness check of its own.

lk_mul.hip keeps every argument check in checker functions that the entry point calls before the first HIP call (the shape guards
are a function of their own, shared with lk_mul_variant, which reports under its caller's name).  Without a device a call that
passes its checker ends in LK_ELAUNCH, or in LK_OK when there are no rows.

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

VJP = "lk_mul_vjp_f32"
# five buffers far from each other and from the probe's own: no probe of an extent meets the overlap guard
G, A, B, DA, DB = (1 << 62) + (0 << 56), (1 << 62) + (1 << 56), (1 << 62) + (2 << 56), (1 << 62) + (3 << 56), (1 << 62) + (4 << 56)
I30 = (1 << 30) - 1
# a row gate: g [2][4][16], a [4][16], b [4], da [2][4][16], db [2][4]
_V = dict(g=G, a=A, b=B, S=2, R=4, L=16, b_row=1, da=DA, db=DB)
_NEAR = dict(g="same", a=A, b=B, da="other", db=DB)  # g at the buffer, da 4096 bytes on
ROWS = [
    *[R(VJP, _V, None, {name: None}, f"{VJP}: null pointer") for name in ("g", "a", "b")],
    # one output may be null, not both
    R(VJP, _V, {"da": None}, {"da": None, "db": None}, f"{VJP}: no output"),
    R(VJP, _V, {"db": None}, {"da": None, "db": None}, f"{VJP}: no output"),
    # b_row is 0 or 1
    R(VJP, _V, {"b_row": 0}, {"b_row": -1}, f"{VJP}: b_row must be"),
    R(VJP, _V, {"b_row": 1}, {"b_row": 2}, f"{VJP}: b_row must be"),
    # 1 <= S
    R(VJP, _V, {"S": 1}, {"S": 0}, f"{VJP}: extent out of range (1 <= S"),
    # 0 <= R; no rows: LK_OK before any HIP call
    R(VJP, _V, {"R": 0}, {"R": -1}, f"{VJP}: extent out of range (1 <= S"),
    # 1 <= L < 2^30
    R(VJP, _V, {"L": 1}, {"L": 0}, f"{VJP}: extent out of range (1 <= S"),
    R(VJP, _V, {"L": I30, "S": 1, "R": 1}, {"L": 1 << 30, "S": 1, "R": 1}, f"{VJP}: extent out of range (1 <= S"),
    # S * R * L < 2^40, approached along each factor
    R(VJP, _V, {"S": (1 << 30) - 1, "R": 1, "L": 1024}, {"S": 1 << 30, "R": 1, "L": 1024}, f"{VJP}: extent out of range (S * R * L"),
    R(VJP, _V, {"S": 1, "R": (1 << 30) - 1, "L": 1024}, {"S": 1, "R": 1 << 30, "L": 1024}, f"{VJP}: extent out of range (S * R * L"),
    R(VJP, _V, {"S": 1 << 5, "R": 1 << 5, "L": I30}, {"S": 1 << 5, "R": 1 << 6, "L": I30}, f"{VJP}: extent out of range (S * R * L"),
    R(VJP, _V, {"S": (1 << 40) - 1, "R": 1, "L": 1, "b_row": 0}, {"S": 1 << 40, "R": 1, "L": 1, "b_row": 0},
      f"{VJP}: extent out of range (S * R * L"),
    # an output must not overlap an input.  g (S R L floats) at the buffer and da 4096 bytes on: 2 x 32 x 16 floats fit exactly
    R(VJP, {**_V, **_NEAR}, {"da": "other"}, {"da": "same"}, f"{VJP}: an output overlaps an input"),
    R(VJP, {**_V, **_NEAR}, {"R": 32}, {"R": 33}, f"{VJP}: an output overlaps an input"),
    # a (R L floats) at the buffer, da 4096 bytes on: 64 rows of 16 floats fit exactly; b ([R]): 1024 rows
    R(VJP, {**_V, "a": "same", "da": "other"}, {"R": 64}, {"R": 65}, f"{VJP}: an output overlaps an input"),
    R(VJP, {**_V, "b": "same", "da": "other"}, {"R": 1024}, {"R": 1025}, f"{VJP}: an output overlaps an input"),
    # the full form's b is [R][L]: 64 rows
    R(VJP, {**_V, "b": "same", "da": "other", "b_row": 0}, {"R": 64}, {"R": 65}, f"{VJP}: an output overlaps an input"),
    # db of a row gate is [S][R]: at the buffer with g 4096 bytes on, 2 x 512 floats fit exactly; the full form's db is [S][R][L]
    R(VJP, {**_V, "db": "same", "g": "other"}, {"R": 512}, {"R": 513}, f"{VJP}: an output overlaps an input"),
    R(VJP, {**_V, "db": "same", "g": "other", "b_row": 0}, {"R": 32}, {"R": 33}, f"{VJP}: an output overlaps an input"),
    R(VJP, {**_V, "db": "same", "a": "other", "da": None}, {"R": 512}, {"R": 513}, f"{VJP}: an output overlaps an input"),
    # the outputs must not overlap each other: da (S R L floats) at the buffer and db 4096 bytes on, and the other way round
    R(VJP, {**_V, "da": "same", "db": "other"}, {"R": 32}, {"R": 33}, f"{VJP}: da overlaps db"),
    R(VJP, {**_V, "db": "same", "da": "other"}, {"R": 512}, {"R": 513}, f"{VJP}: da overlaps db"),
    R(VJP, {**_V, "da": "same", "db": "same"}, {"db": "other"}, {"db": "same"}, f"{VJP}: da overlaps db"),
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
    return ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items())[:80] + f"#{i}"


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")
    assert [p[2] for p in protos[VJP]] == ["g", "a", "b", "S", "R", "L", "b_row", "da", "db", "stream"]
    assert [p[2] for p in protos["lk_mul_variant"]] == ["S", "R", "L", "b_row", "want_da", "want_db", "aligned"]


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
        if {**row["base"], **row["accept"]}["R"] == 0:
            assert rc == LK_OK  # (no rows: the call returns before any HIP call)


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_mul.hip")).read()
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
    """every LK_REQUIRE of lk_mul.hip: a row's first-refused call came back with that guard's message (the guards of the shared
    shape checker - their literal starts with "%s: " - under the entry point's name)"""
    messages = _guard_messages()
    assert len(messages) == 7, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = [VJP + m[2:] if m.startswith("%s: ") else m for m in messages]
    assert all(m.startswith(VJP + ": ") for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_point_checks_through_its_checker_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_mul.hip")).read()
    body = text[text.index(f'extern "C" int {VJP}'):]
    body = body[:body.index("\n}\n")]
    assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
    assert body.index("mul_check(") < body.index("if (R == 0) return LK_OK") < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {VJP, "lk_mul_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_is_negative_exactly_where_the_entry_point_refuses():
    """lk_mul_variant is host code: every shape row of the table, asked in this process - a dict on the accepted side, None on the
    refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if any(f in row["fragment"] for f in ("null pointer", "overlaps")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            got = K.mul_variant(a["S"], a["R"], a["L"], a["b_row"], (a["da"] is not None, a["db"] is not None))
            assert (got is not None) == want, (side, row[side], got)
            asked += 1
    assert asked >= 24
    lib = K.lib
    assert lib.lk_mul_variant(2, 4, 16, 2, 1, 1, 1) == -1 and lib.lk_mul_variant(2, 4, 16, 1, 0, 0, 1) == -1
    assert lib.lk_mul_variant(2, 4, 16, 1, 1, 0, 1) >= 0


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
