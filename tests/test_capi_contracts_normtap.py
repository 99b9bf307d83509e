"""The argument contract of lk_jac_norm_affine_nhwc_f16x2 and lk_normtap_variant (csrc/lk_normtap.hip), probed at its edges WITHOUT a
device - the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_dwconv.py: a table of
last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_normtap.hip keeps every argument check in checker functions that the entry point calls before the first HIP call (the shape
guards are one function, shared with the variant query, which reports under its caller's name).  Without a device a call that
passes its checker ends in LK_ELAUNCH, or in LK_OK for an empty batch or when both column blocks are absent.
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

FN = "lk_jac_norm_affine_nhwc_f16x2"
_B = dict(S=3, B=2, L=5, Ch=8, P=21, wcol0=0, bcol0=8)
I31, I30 = (1 << 31) - 1, (1 << 30) - 1
ONE = dict(S=1, B=1, L=1, Ch=1, P=2, wcol0=0, bcol0=1)  # one element: the count guard stays out of an extent's way
ROWS = [
    R(FN, _B, None, {"g_h": None}, f"{FN}: null pointer"),
    R(FN, _B, None, {"g_l": None}, f"{FN}: null pointer"),
    R(FN, _B, None, {"sexp": None}, f"{FN}: null pointer"),
    R(FN, _B, None, {"x": None}, f"{FN}: null pointer"),
    R(FN, _B, None, {"Js": None}, f"{FN}: null pointer"),
    # mu and rstd: both or neither
    R(FN, _B, {"mu": None, "rstd": None}, {"mu": None}, f"{FN}: mu and rstd are given together or not at all"),
    R(FN, _B, {"mu": "other", "rstd": "other"}, {"rstd": None}, f"{FN}: mu and rstd are given together or not at all"),
    R(FN, _B, {"S": 1}, {"S": 0}, f"{FN}: extent out of range"),
    R(FN, _B, {"B": 0}, {"B": -1}, f"{FN}: extent out of range"),
    R(FN, _B, {"L": 1}, {"L": 0}, f"{FN}: extent out of range"),
    R(FN, _B, {"Ch": 1, "bcol0": 1}, {"Ch": 0}, f"{FN}: extent out of range"),
    R(FN, _B, {**ONE, "S": I31}, {**ONE, "S": 1 << 31}, f"{FN}: extent out of range"),
    R(FN, _B, {**ONE, "B": I31}, {**ONE, "B": 1 << 31}, f"{FN}: extent out of range"),
    # S * B < 2^31
    R(FN, _B, {**ONE, "S": 1 << 16, "B": (1 << 15) - 1}, {**ONE, "S": 1 << 16, "B": 1 << 15}, f"{FN}: extent out of range"),
    R(FN, _B, {**ONE, "L": I30}, {**ONE, "L": 1 << 30}, f"{FN}: extent out of range"),
    R(FN, _B, {**ONE, "Ch": I30, "P": 1 << 31, "bcol0": 1 << 30}, {**ONE, "Ch": 1 << 30, "P": 1 << 32, "bcol0": 1 << 31},
      f"{FN}: extent out of range"),
    # S * B * L * Ch < 2^40: 2^10 positions x 2^10 channels x 2^20 images
    R(FN, _B, {"S": 1, "B": (1 << 20) - 1, "L": 1 << 10, "Ch": 1 << 10, "P": 1 << 11, "bcol0": 1 << 10},
      {"S": 1, "B": 1 << 20, "L": 1 << 10, "Ch": 1 << 10, "P": 1 << 11, "bcol0": 1 << 10}, f"{FN}: too many elements"),
    # B * (channel tiles per sample) < 2^31: 2^20 channels on an odd address are 2^14 tiles of 64 one-channel lanes
    R(FN, _B, {"S": 1, "L": 1, "B": (1 << 17) - 1, "Ch": 1 << 20, "P": 1 << 21, "bcol0": 1 << 20, "x": "odd"},
      {"S": 1, "L": 1, "B": 1 << 17, "Ch": 1 << 20, "P": 1 << 21, "bcol0": 1 << 20, "x": "odd"},
      f"{FN}: too many channel tiles for one launch"),
    # the column blocks: inside P ...
    R(FN, _B, {"bcol0": 13}, {"bcol0": 14}, f"{FN}: column range outside Js"),
    R(FN, _B, {"wcol0": 13, "bcol0": 0}, {"wcol0": 14, "bcol0": 0}, f"{FN}: column range outside Js"),
    R(FN, _B, {"P": 16}, {"P": 15}, f"{FN}: column range outside Js"),
    # ... and apart; a negative offset skips its block, whatever else it would overlap
    R(FN, _B, {"bcol0": 8}, {"bcol0": 7}, f"{FN}: weight and bias columns overlap"),
    R(FN, _B, {"wcol0": 8, "bcol0": 0}, {"wcol0": 7, "bcol0": 0}, f"{FN}: weight and bias columns overlap"),
    R(FN, _B, {"wcol0": -1, "bcol0": 0}, {"wcol0": 0, "bcol0": 0}, f"{FN}: weight and bias columns overlap"),
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
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")


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
        if a["B"] == 0 or (a["wcol0"] < 0 and a["bcol0"] < 0):
            assert rc == LK_OK  # (nothing to write: returns before any HIP call)


def test_nothing_to_write_returns_ok_before_any_hip_call():
    """an empty batch, and both column blocks absent, in THIS process (host code only; the pointers are never read)"""
    P = _Probe()
    assert P.call(FN, {**_B, "B": 0})[0] == LK_OK
    assert P.call(FN, {**_B, "wcol0": -1, "bcol0": -1})[0] == LK_OK
    assert P.call(FN, {**_B, "wcol0": -5, "bcol0": -1, "P": 0})[0] == LK_OK


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_normtap.hip")).read()
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
    """every LK_REQUIRE of lk_normtap.hip (their literals start with "%s: "): a row's first-refused call came back with that
    guard's message under the entry point's name"""
    messages = _guard_messages()
    assert len(messages) >= 7 and all(m.startswith("%s: ") for m in messages), messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    missing = [m for m in (FN + msg[2:] for msg in messages) if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_point_checks_through_its_checker_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_normtap.hip")).read()
    body = text[text.index(f'extern "C" int {FN}'):]
    body = body[:body.index("\n}\n")]
    assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
    assert body.index("normtap_check(") < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FN, "lk_normtap_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_point_refuses():
    """lk_normtap_variant is host code: every row of the table that is about the shape, asked in this process - a dict on the
    accepted side, None on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if not any(f in row["fragment"] for f in ("extent out of range", "too many")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            r = K.lib.lk_normtap_variant(*[int(a[n]) for n in ("S", "B", "L", "Ch")], 1, int(a.get("x") != "odd"))
            assert (r >= 0) == want, (side, row[side], r)
            asked += 1
    assert asked >= 20
    assert K.normtap_variant(9, 128, 1024, 64) == {"vec": 8, "seed_split": True, "affine": True, "seeds_per_pass": 4, "lane_rows": 32,
                                                   "seeds_per_slice": 3, "channel_tiles": 1}
    assert K.normtap_variant(9, 128, 16, 512, affine=False) == {"vec": 8, "seed_split": True, "affine": False, "seeds_per_pass": 4,
                                                                "lane_rows": 8, "seeds_per_slice": 5, "channel_tiles": 2}
    assert K.normtap_variant(9, 1024, 16, 64, aligned=False) == {"vec": 1, "seed_split": False, "affine": True, "seeds_per_pass": 8,
                                                                 "lane_rows": 4, "seeds_per_slice": 9, "channel_tiles": 1}
    assert K.normtap_variant(9, 128, 1 << 30, 64) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
