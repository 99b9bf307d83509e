"""The argument contracts of lk_slice_fwd_f32, lk_slice_vjp_f32 and lk_slice_variant (csrc/lk_slice.hip), probed at their edges
WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_cat.py: a
table of last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_slice.hip keeps every argument check in checker functions that the entry points call before the first HIP call (the extent and
range guards are functions of their own, which report under their caller's name).  Without a device a call that passes its checker
ends in LK_ELAUNCH, or in LK_OK when there are no rows.

The VJP takes HOST arrays: of device pointers - a table entry ``("parr", [...])`` stands for such an array, its entries "same" (the
probe's buffer), "other" (4096 bytes on), "far" (2^61), an integer address or None - and of 64-bit column ranges (plain lists).
"""
import ctypes
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

FWD, VJP = "lk_slice_fwd_f32", "lk_slice_vjp_f32"
FAR = 1 << 62  # (an address nothing else is near: no probe of an extent meets the overlap guard)
I30 = (1 << 30) - 1


def parr(*entries):
    return ("parr", list(entries))


# src: 4 x 16 floats = 256 bytes at the buffer; dst 4 x 8 floats 4096 bytes on
_F = dict(src="same", dst="other", R=4, Ct=16, c0=4, Cs=8)
# two pieces - an fp32 map of columns [4, 12) at the buffer (4 x 8 floats = 128 bytes), a full-width split tensor far away -, dst
# 4 x 16 floats 4096 bytes on
_V = dict(npieces=2, f32=parr("same", None), hi=parr(None, "far"), lo=parr(None, "far"), sexp=parr(None, "far"), c0=[4, 0],
          cs=[8, 16], R=4, Ct=16, dst="other", amax=None)
_FARV = {"dst": FAR, "f32": parr("far", None)}
ROWS = [
    # ---- the forward -----------------------------------------------------------------------------------------------------------
    R(FWD, _F, None, {"src": None}, f"{FWD}: null pointer"),
    R(FWD, _F, None, {"dst": None}, f"{FWD}: null pointer"),
    # 1 <= Cs
    R(FWD, _F, {"Cs": 1}, {"Cs": 0}, f"{FWD}: slice out of range"),
    # 0 <= c0
    R(FWD, _F, {"c0": 0}, {"c0": -1}, f"{FWD}: slice out of range"),
    # c0 + Cs <= Ct: the slice may end with the row
    R(FWD, _F, {"c0": 8, "Cs": 8}, {"c0": 9, "Cs": 8}, f"{FWD}: slice out of range"),
    R(FWD, _F, {"c0": 0, "Cs": 16}, {"c0": 0, "Cs": 17}, f"{FWD}: slice out of range"),
    R(FWD, _F, {"c0": 15, "Cs": 1}, {"c0": 16, "Cs": 1}, f"{FWD}: slice out of range"),
    # 1 <= Ct < 2^30
    R(FWD, _F, {"Ct": 1, "c0": 0, "Cs": 1}, {"Ct": 0, "c0": 0, "Cs": 1}, f"{FWD}: row length out of range"),
    R(FWD, _F, {"Ct": I30, "R": 1, "c0": I30 - 1, "Cs": 1, "dst": FAR}, {"Ct": 1 << 30, "R": 1, "c0": I30 - 1, "Cs": 1, "dst": FAR},
      f"{FWD}: row length out of range"),
    # 0 <= R; no rows: LK_OK before any HIP call
    R(FWD, _F, {"R": 0}, {"R": -1}, f"{FWD}: extent out of range"),
    # R * Ct < 2^40
    R(FWD, _F, {"R": (1 << 30) - 1, "Ct": 1024, "dst": FAR}, {"R": 1 << 30, "Ct": 1024, "dst": FAR}, f"{FWD}: extent out of range"),
    R(FWD, _F, {"R": (1 << 40) - 1, "Ct": 1, "c0": 0, "Cs": 1, "dst": FAR}, {"R": 1 << 40, "Ct": 1, "c0": 0, "Cs": 1, "dst": FAR},
      f"{FWD}: extent out of range"),
    # dst must not overlap src.  src at the buffer and dst 4096 bytes on: 64 rows of 16 floats of src fit exactly, one more does
    # not; the other way round 128 rows of 8 floats of dst fit exactly
    R(FWD, _F, {"dst": "other"}, {"dst": "same"}, f"{FWD}: dst overlaps src"),
    R(FWD, _F, {"R": 64}, {"R": 65}, f"{FWD}: dst overlaps src"),
    R(FWD, _F, {"src": "other", "dst": "same", "R": 128}, {"src": "other", "dst": "same", "R": 129}, f"{FWD}: dst overlaps src"),
    # ---- the VJP ---------------------------------------------------------------------------------------------------------------
    # 1 <= npieces <= 8
    R(VJP, _V, {"npieces": 1}, {"npieces": 0}, f"{VJP}: npieces out of range"),
    R(VJP, _V, {"npieces": 8, "f32": parr("same", None, *["same"] * 6), "hi": parr(None, "far", *[None] * 6),
                "lo": parr(None, "far", *[None] * 6), "sexp": parr(None, "far", *[None] * 6), "c0": [4, 0] + [4] * 6,
                "cs": [8, 16] + [8] * 6},
      {"npieces": 9, "f32": parr(*["same"] * 9), "hi": parr(*[None] * 9), "lo": parr(*[None] * 9), "sexp": parr(*[None] * 9),
       "c0": [4] * 9, "cs": [8] * 9}, f"{VJP}: npieces out of range"),
    # the six host arrays and dst
    *[R(VJP, _V, None, {name: None}, f"{VJP}: null pointer") for name in ("f32", "hi", "lo", "sexp", "c0", "cs", "dst")],
    # a piece: f32, or all three of hi, lo and sexp (what stands in the other arrays is not looked at)
    R(VJP, _V, {"f32": parr("same", "far")}, {"hi": parr(None, None)}, f"{VJP}: a piece is an fp32 map"),
    R(VJP, _V, {"hi": parr("far", "far")}, {"lo": parr(None, None)}, f"{VJP}: a piece is an fp32 map"),
    R(VJP, _V, {"npieces": 1}, {"sexp": parr(None, None)}, f"{VJP}: a piece is an fp32 map"),
    # 1 <= cs[p], 0 <= c0[p], c0[p] + cs[p] <= Ct - of the first piece and of the last
    R(VJP, _V, {"cs": [1, 16]}, {"cs": [0, 16]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"c0": [4, 15], "cs": [8, 1]}, {"c0": [4, 15], "cs": [8, 0]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"c0": [0, 0]}, {"c0": [-1, 0]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"c0": [4, 0]}, {"c0": [4, -1]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"c0": [8, 0]}, {"c0": [9, 0]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"cs": [8, 16]}, {"cs": [8, 17]}, f"{VJP}: slice out of range"),
    R(VJP, _V, {"c0": [4, 15], "cs": [8, 1]}, {"c0": [4, 16], "cs": [8, 1]}, f"{VJP}: slice out of range"),
    # 1 <= Ct < 2^30
    R(VJP, _V, {"Ct": 1, "c0": [0, 0], "cs": [1, 1]}, {"Ct": 0, "c0": [0, 0], "cs": [1, 1]}, f"{VJP}: row length out of range"),
    R(VJP, _V, {"Ct": I30, "R": 1, "c0": [I30 - 1, 0], "cs": [1, 1], **_FARV},
      {"Ct": 1 << 30, "R": 1, "c0": [I30 - 1, 0], "cs": [1, 1], **_FARV}, f"{VJP}: row length out of range"),
    # 0 <= R; no rows: LK_OK before any HIP call
    R(VJP, _V, {"R": 0}, {"R": -1}, f"{VJP}: extent out of range"),
    # R * Ct < 2^40
    R(VJP, _V, {"R": (1 << 30) - 1, "Ct": 1024, **_FARV}, {"R": 1 << 30, "Ct": 1024, **_FARV}, f"{VJP}: extent out of range"),
    R(VJP, _V, {"R": (1 << 40) - 1, "Ct": 1, "c0": [0, 0], "cs": [1, 1], **_FARV},
      {"R": 1 << 40, "Ct": 1, "c0": [0, 0], "cs": [1, 1], **_FARV}, f"{VJP}: extent out of range"),
    # dst must not overlap a piece.  An fp32 piece of 8 columns at the buffer and dst 4096 bytes on: 128 rows fit exactly; a plane
    # of 16 halves a row: 128 rows; dst (16 floats a row) at the buffer and the piece 4096 bytes on: 64 rows of dst fit exactly
    R(VJP, _V, {"dst": "other"}, {"dst": "same"}, f"{VJP}: dst overlaps a piece"),
    R(VJP, _V, {"R": 128}, {"R": 129}, f"{VJP}: dst overlaps a piece"),
    R(VJP, _V, {"f32": parr("far", None), "hi": parr(None, "same"), "R": 128}, {"f32": parr("far", None), "hi": parr(None, "same"), "R": 129},
      f"{VJP}: dst overlaps a piece"),
    R(VJP, _V, {"f32": parr("far", None), "lo": parr(None, "same"), "R": 128}, {"f32": parr("far", None), "lo": parr(None, "same"), "R": 129},
      f"{VJP}: dst overlaps a piece"),
    R(VJP, _V, {"f32": parr("other", None), "dst": "same", "R": 64}, {"f32": parr("other", None), "dst": "same", "R": 65},
      f"{VJP}: dst overlaps a piece"),
]
SENTINEL = ("lk_symmetrize_f32", {"n": -1})


def _resolve(P, values):
    """host arrays of pointers for the ``("parr", [...])`` entries (kept alive by the probe)"""
    out = {}
    for k, v in values.items():
        if isinstance(v, (tuple, list)) and len(v) == 2 and v[0] == "parr":
            where = {"same": P.buf, "other": P.buf + 4096, "far": 1 << 61, None: None}
            arr = (ctypes.c_void_p * max(len(v[1]), 1))(*[where.get(e, e) if not isinstance(e, int) else e for e in v[1]])
            P.keep.append(arr)
            v = ctypes.addressof(arr)
        out[k] = v
    return out


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
            rc, msg = P.call(row["fn"], _resolve(P, {**row["base"], **row[side]}))
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
    return (ROWS[i]["fn"][9:12] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items()))[:100]


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")
    assert [p[2] for p in protos[FWD]] == ["src", "R", "Ct", "c0", "Cs", "dst", "stream"]
    assert [p[2] for p in protos[VJP]] == ["npieces", "f32", "hi", "lo", "sexp", "c0", "cs", "R", "Ct", "dst", "amax", "stream"]
    assert [p[2] for p in protos["lk_slice_variant"]] == ["npieces", "split_mask", "c0", "cs", "R", "Ct", "aligned"]


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
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_slice.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for m in re.finditer(r"LK_REQUIRE\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', text[m.end():j])))
    return out


def test_every_guard_of_the_file_is_reached_by_a_row_under_both_names(probes):
    """every LK_REQUIRE of lk_slice.hip: a row's first-refused call came back with that guard's message - the guards of the shared
    checkers (their literal starts with "%s: ") under the name of EITHER entry point"""
    messages = _guard_messages()
    assert len(messages) == 9, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = []
    for msg in messages:
        want += [fn + msg[2:] for fn in (FWD, VJP)] if msg.startswith("%s: ") else [msg]
    assert all(m.startswith((FWD + ": ", VJP + ": ")) for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_slice.hip")).read()
    for fn, checker in ((FWD, "slice_check_fwd("), (VJP, "slice_check_vjp(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FWD, VJP, "lk_slice_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_points_refuse():
    """lk_slice_variant is host code: every numeric row of the VJP's table, asked in this process - a dict on the accepted side,
    None on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if row["fn"] != VJP or any(f in row["fragment"] for f in ("null pointer", "overlaps", "a piece is")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            n = int(a["npieces"])
            mask = sum(1 << i for i, e in enumerate(a["f32"][1][:n]) if e is None)
            got = K.slice_variant(mask, a["c0"][:max(n, 0)] if 0 <= n <= 8 else a["c0"], a["cs"][:max(n, 0)] if 0 <= n <= 8 else a["cs"],
                                  a["R"], a["Ct"])
            assert (got is not None) == want, (side, row[side], got)
            asked += 1
    assert asked >= 25
    assert K.slice_variant(2, [0, 32], [32, 32], 9 * 128 * 32 * 32, 64) == {"vec": True, "npieces": 2, "split_mask": 2,
                                                                            "wide_index": False, "blocks": 2048}
    assert K.slice_variant(2, [0, 32], [32, 33], 4, 64) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
