"""The argument contracts of lk_softmax_vjp_f32 / lk_softmax_vjp_variant (csrc/lk_softmax.hip) and lk_matmul_vjp_f32 /
lk_matmul_vjp_variant (csrc/lk_matmul.hip), probed at their edges WITHOUT a device - the method of tests/test_capi_contracts.py (whose
helpers are reused) and tests/test_capi_contracts_mul.py: a table of last-accepted / first-refused values, a child process that sees
no device, and a completeness check of its own.

Both files keep every argument check in checker functions that the entry point calls before the first HIP call (the shape guards
are a function of their own, shared with the ``*_variant`` query, which reports under its caller's name).  Without a device a call
that passes its checker ends in LK_ELAUNCH, or in LK_OK when there are no rows / no sample matrices.

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

SMX, MM = "lk_softmax_vjp_f32", "lk_matmul_vjp_f32"
FILES = {SMX: "lk_softmax.hip", MM: "lk_matmul.hip"}
VARIANT = {SMX: "lk_softmax_vjp_variant", MM: "lk_matmul_vjp_variant"}
CHECKER = {SMX: "softmax_check(", MM: "matmul_check("}
EMPTY = {SMX: ("R", "if (R == 0) return LK_OK"), MM: ("NB", "if (NB == 0) return LK_OK")}
N_GUARDS = {SMX: 5, MM: 7}
# five buffers far from each other and from the probe's own: no probe of an extent meets the overlap guard
G, A, B, DA, DB = (1 << 62) + (0 << 56), (1 << 62) + (1 << 56), (1 << 62) + (2 << 56), (1 << 62) + (3 << 56), (1 << 62) + (4 << 56)
I30, I24 = (1 << 30) - 1, (1 << 24) - 1
# softmax: g [2][4][16], y [4][16], dx [2][4][16]
_S = dict(g=G, y=A, S=2, R=4, L=16, is_log=0, dx=DA)
# matmul: g [2][4][4][4], a [4][4][4], b [4][4][4], da [2][4][4][4], db [2][4][4][4]: 128 NB bytes of g, da and db, 64 NB of a and b
_M = dict(g=G, a=A, b=B, S=2, NB=4, M=4, K=4, N=4, da=DA, db=DB)
_ONE = dict(S=1, NB=1, M=1, K=1, N=1)
_X = f"{MM}: extent out of range (1 <= S"
_P = f"{MM}: extent out of range (S * NB"
ROWS = [
    # ---- lk_softmax_vjp_f32 ------------------------------------------------------------------------------------------------------
    *[R(SMX, _S, None, {name: None}, f"{SMX}: null pointer") for name in ("g", "y", "dx")],
    R(SMX, _S, {"is_log": 0}, {"is_log": -1}, f"{SMX}: is_log must be"),
    R(SMX, _S, {"is_log": 1}, {"is_log": 2}, f"{SMX}: is_log must be"),
    R(SMX, _S, {"S": 1}, {"S": 0}, f"{SMX}: extent out of range (1 <= S"),
    R(SMX, _S, {"R": 0}, {"R": -1}, f"{SMX}: extent out of range (1 <= S"),  # no rows: LK_OK before any HIP call
    R(SMX, _S, {"L": 1}, {"L": 0}, f"{SMX}: extent out of range (1 <= S"),
    R(SMX, _S, {"L": I30, "S": 1, "R": 1}, {"L": 1 << 30, "S": 1, "R": 1}, f"{SMX}: extent out of range (1 <= S"),
    # S * R * L < 2^40, approached along each factor
    R(SMX, _S, {"S": (1 << 30) - 1, "R": 1, "L": 1024}, {"S": 1 << 30, "R": 1, "L": 1024}, f"{SMX}: extent out of range (S * R * L"),
    R(SMX, _S, {"S": 1, "R": (1 << 30) - 1, "L": 1024}, {"S": 1, "R": 1 << 30, "L": 1024}, f"{SMX}: extent out of range (S * R * L"),
    R(SMX, _S, {"S": 1 << 5, "R": 1 << 5, "L": I30}, {"S": 1 << 5, "R": 1 << 6, "L": I30}, f"{SMX}: extent out of range (S * R * L"),
    # dx must not overlap an input: g (S R L floats) at the buffer and dx 4096 bytes on: 2 x 32 x 16 floats fit exactly; y: 64 rows
    R(SMX, {**_S, "g": "same", "dx": "other"}, {"dx": "other"}, {"dx": "same"}, f"{SMX}: dx overlaps an input"),
    R(SMX, {**_S, "g": "same", "dx": "other"}, {"R": 32}, {"R": 33}, f"{SMX}: dx overlaps an input"),
    R(SMX, {**_S, "y": "same", "dx": "other"}, {"R": 64}, {"R": 65}, f"{SMX}: dx overlaps an input"),
    R(SMX, {**_S, "dx": "same", "g": "other"}, {"R": 32}, {"R": 33}, f"{SMX}: dx overlaps an input"),
    R(SMX, {**_S, "dx": "same", "y": "other"}, {"R": 32}, {"R": 33}, f"{SMX}: dx overlaps an input"),
    # ---- lk_matmul_vjp_f32 -------------------------------------------------------------------------------------------------------
    *[R(MM, _M, None, {name: None}, f"{MM}: null pointer") for name in ("g", "a", "b")],
    # one output may be null, not both
    R(MM, _M, {"da": None}, {"da": None, "db": None}, f"{MM}: no output"),
    R(MM, _M, {"db": None}, {"da": None, "db": None}, f"{MM}: no output"),
    R(MM, _M, {"S": 1}, {"S": 0}, _X),
    R(MM, _M, {"NB": 0}, {"NB": -1}, _X),  # no sample matrices: LK_OK before any HIP call
    *[R(MM, _M, {d: 1}, {d: 0}, _X) for d in ("M", "K", "N")],
    *[R(MM, {**_M, **_ONE}, {d: I24}, {d: 1 << 24}, _X) for d in ("M", "K", "N")],
    # S * NB * M * N, S * NB * M * K and S * NB * K * N < 2^40, each alone and along S and NB
    R(MM, {**_M, **_ONE, "M": 1024, "N": 1024}, {"S": (1 << 20) - 1}, {"S": 1 << 20}, _P),
    R(MM, {**_M, **_ONE, "M": 1024, "K": 1024}, {"S": (1 << 20) - 1}, {"S": 1 << 20}, _P),
    R(MM, {**_M, **_ONE, "K": 1024, "N": 1024}, {"NB": (1 << 20) - 1}, {"NB": 1 << 20}, _P),
    # the tiles of grid.x: NB * ceil(M / 64) * ceil(K / 64) and NB * ceil(K / 64) * ceil(N / 64) < 2^31
    R(MM, {**_M, **_ONE}, {"NB": (1 << 31) - 1}, {"NB": 1 << 31}, f"{MM}: too many tiles"),
    R(MM, {**_M, **_ONE, "M": 65}, {"NB": (1 << 30) - 1}, {"NB": 1 << 30}, f"{MM}: too many tiles"),
    R(MM, {**_M, **_ONE, "N": 65}, {"NB": (1 << 30) - 1}, {"NB": 1 << 30}, f"{MM}: too many tiles"),
    # an output must not overlap an input: g at the buffer and da 4096 bytes on: 32 sample matrices fit exactly; a, b: 64
    R(MM, {**_M, "g": "same", "da": "other"}, {"da": "other"}, {"da": "same"}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "g": "same", "da": "other"}, {"NB": 32}, {"NB": 33}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "a": "same", "da": "other"}, {"NB": 64}, {"NB": 65}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "b": "same", "db": "other"}, {"NB": 64}, {"NB": 65}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "b": "same", "da": "other", "db": None}, {"NB": 64}, {"NB": 65}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "da": "same", "g": "other"}, {"NB": 32}, {"NB": 33}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "db": "same", "a": "other", "da": None}, {"NB": 32}, {"NB": 33}, f"{MM}: an output overlaps an input"),
    # rectangular extents: da is [S][NB][M][K] and db [S][NB][K][N] (K = 8: 256 NB bytes each against 128 NB of g)
    R(MM, {**_M, "K": 8, "da": "same", "g": "other"}, {"NB": 16}, {"NB": 17}, f"{MM}: an output overlaps an input"),
    R(MM, {**_M, "K": 8, "g": "same", "db": "other"}, {"NB": 32}, {"NB": 33}, f"{MM}: an output overlaps an input"),
    # the outputs must not overlap each other
    R(MM, {**_M, "da": "same", "db": "other"}, {"NB": 32}, {"NB": 33}, f"{MM}: da overlaps db"),
    R(MM, {**_M, "db": "same", "da": "other"}, {"NB": 32}, {"NB": 33}, f"{MM}: da overlaps db"),
    R(MM, {**_M, "da": "same", "db": "same"}, {"db": "other"}, {"db": "same"}, f"{MM}: da overlaps db"),
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
    assert [p[2] for p in protos[SMX]] == ["g", "y", "S", "R", "L", "is_log", "dx", "stream"]
    assert [p[2] for p in protos[VARIANT[SMX]]] == ["S", "R", "L", "is_log", "aligned"]
    assert [p[2] for p in protos[MM]] == ["g", "a", "b", "S", "NB", "M", "K", "N", "da", "db", "stream"]
    assert [p[2] for p in protos[VARIANT[MM]]] == ["S", "NB", "M", "K", "N", "want_da", "want_db"]


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
        if {**row["base"], **row["accept"]}[EMPTY[row["fn"]][0]] == 0:
            assert rc == LK_OK  # (nothing to do: the call returns before any HIP call)


def _guard_messages(fn):
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", FILES[fn])).read()
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for m in re.finditer(r"LK_REQUIRE\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', text[m.end():j])))
    return out


@pytest.mark.parametrize("fn", (SMX, MM))
def test_every_guard_of_the_file_is_reached_by_a_row(probes, fn):
    """every LK_REQUIRE of the file: a row's first-refused call came back with that guard's message (the guards of the shared shape
    checker - their literal starts with "%s: " - under the entry point's name)"""
    messages = _guard_messages(fn)
    assert len(messages) == N_GUARDS[fn], messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS)) if ROWS[i]["fn"] == fn}
    want = [fn + m[2:] if m.startswith("%s: ") else m for m in messages]
    assert all(m.startswith(fn + ": ") for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


@pytest.mark.parametrize("fn", (SMX, MM))
def test_the_entry_point_checks_through_its_checker_only(fn):
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", FILES[fn])).read()
    body = text[text.index(f'extern "C" int {fn}'):]
    body = body[:body.index("\n}\n")]
    assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
    assert body.index(CHECKER[fn]) < body.index(EMPTY[fn][1]) < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {fn, VARIANT[fn]} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_queries_are_negative_exactly_where_the_entry_points_refuse():
    """the ``*_variant`` queries are host code: every shape row of the table, asked in this process - a dict on the accepted side,
    None on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if any(f in row["fragment"] for f in ("null pointer", "overlaps")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            if row["fn"] == SMX:
                got = K.lib.lk_softmax_vjp_variant(a["S"], a["R"], a["L"], a["is_log"], 1) >= 0
            else:
                got = K.matmul_vjp_variant(a["S"], a["NB"], a["M"], a["K"], a["N"], (a["da"] is not None, a["db"] is not None)) is not None
            assert got == want, (side, row[side], got)
            asked += 1
    assert asked >= 50
    assert K.softmax_vjp_variant(2, 4, 16, True)["log"] and K.softmax_vjp_variant(2, 4, 16, False, aligned=False)["vec"] is False
    assert K.lib.lk_matmul_vjp_variant(2, 4, 4, 4, 4, 0, 0) == -1 and K.lib.lk_matmul_vjp_variant(2, 4, 4, 4, 4, 1, 0) >= 0


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
