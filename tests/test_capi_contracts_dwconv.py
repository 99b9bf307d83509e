"""The argument contracts of lk_dwconv_fwd_nhwc_f32, lk_dwconv_bwd_nhwc_f16x2 and lk_dwconv_variant (csrc/lk_dwconv.hip), probed at
their edges WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and
tests/test_capi_contracts_pool.py: a table of last-accepted / first-refused values, a child process that sees no device, and a
completeness check of its own.

lk_dwconv.hip keeps every argument check in checker functions that the entry points call before the first HIP call (the shape
guards are one function, which reports under its caller's name).  Without a device a call that passes its checker ends in
LK_ELAUNCH, or in LK_OK for an empty batch.
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

FWD, BWD = "lk_dwconv_fwd_nhwc_f32", "lk_dwconv_bwd_nhwc_f16x2"
_GEO = dict(B=2, H=8, W=8, C=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1)
_F = dict(_GEO)
# (the planes and dx: two places of the probe's buffer, 4096 bytes apart; a plane is 3 * 2 * 8 * 8 * 4 halves = 3072 bytes)
_V = dict(_GEO, g_h="same", g_l="same", dx="other", amax=None, S=3)
I31, I30 = (1 << 31) - 1, (1 << 30) - 1
# one pixel, one channel, one tap: the count guard stays out of an extent's way
ONE = dict(H=1, W=1, C=1, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0)
ROWS = []
for fn, base in ((FWD, _F), (BWD, _V)):
    # dx at an address far from g: nothing is touched without a device, and the overlap guard must not answer a probe of the extents
    far = {"dx": 1 << 62} if fn == BWD else {}
    one_seed = {"S": 1} if fn == BWD else {}
    ROWS += [
        R(fn, base, None, {"w_tap": None}, f"{fn}: null pointer"),
        # kh * kw <= 25: the register cap of the backward (100 weight registers per lane at 5 x 5 x 4 channels)
        R(fn, base, {"kh": 5, "kw": 5}, {"kh": 2, "kw": 13, "W": 16}, f"{fn}: window out of range"),
        R(fn, base, {"kh": 5, "kw": 5}, {"kh": 13, "kw": 2, "H": 16}, f"{fn}: window out of range"),
        R(fn, base, {"kh": 25, "kw": 1, "H": 32, "pw": 0}, {"kh": 26, "kw": 1, "H": 32, "pw": 0}, f"{fn}: window out of range"),
        R(fn, base, {"kw": 25, "kh": 1, "W": 32, "ph": 0}, {"kw": 26, "kh": 1, "W": 32, "ph": 0}, f"{fn}: window out of range"),
        R(fn, base, {"kh": 1, "ph": 0}, {"kh": 0, "ph": 0}, f"{fn}: window out of range"),
        R(fn, base, {"kw": 1, "pw": 0}, {"kw": 0, "pw": 0}, f"{fn}: window out of range"),
        R(fn, base, {"sh": 1}, {"sh": 0}, f"{fn}: stride out of range"),
        R(fn, base, {"sw": 1}, {"sw": 0}, f"{fn}: stride out of range"),
        R(fn, base, {"sh": 8}, {"sh": 9}, f"{fn}: stride out of range"),
        R(fn, base, {"sw": 8}, {"sw": 9}, f"{fn}: stride out of range"),
        # padding below the window: 2 of 3, never 3
        R(fn, base, {"ph": 2}, {"ph": 3}, f"{fn}: padding out of range"),
        R(fn, base, {"pw": 2}, {"pw": 3}, f"{fn}: padding out of range"),
        R(fn, base, {"ph": 0}, {"ph": -1}, f"{fn}: padding out of range"),
        R(fn, base, {"pw": 0}, {"pw": -1}, f"{fn}: padding out of range"),
        R(fn, base, {"B": 0}, {"B": -1}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "H": 32767, **far}, {**ONE, "H": 32768, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "W": 32767, **far}, {**ONE, "W": 32768, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "H": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "W": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "C": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "C": I30, "B": 1, **far}, {**ONE, "C": 1 << 30, "B": 1, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "B": I31, **far, **one_seed}, {**ONE, "B": 1 << 31, **far, **one_seed}, f"{fn}: extent out of range"),
        # OH = (H + 2 ph - kh) / sh + 1 >= 1: a three-row window on one row needs its padding
        R(fn, base, {"H": 1}, {"H": 1, "ph": 0}, f"{fn}: empty output"),
        R(fn, base, {"W": 1}, {"W": 1, "pw": 0}, f"{fn}: empty output"),
        R(fn, base, {"H": 3, "ph": 0}, {"H": 2, "ph": 0}, f"{fn}: empty output"),
        # S * B * C * max(H * W, OH * OW) < 2^40: 2^10 pixels x 2^10 channels x 2^20 images; with a window of 2, stride 1 and
        # padding 1 it is the OUTPUT that has 2^10 pixels (the input has 31 x 31)
        R(fn, base, {"H": 32, "W": 32, "C": 1 << 10, "B": (1 << 20) - 1, **far, **one_seed},
          {"H": 32, "W": 32, "C": 1 << 10, "B": 1 << 20, **far, **one_seed}, f"{fn}: too many elements"),
        R(fn, base, {"H": 31, "W": 31, "kh": 2, "kw": 2, "C": 1 << 10, "B": (1 << 20) - 1, **far, **one_seed},
          {"H": 31, "W": 31, "kh": 2, "kw": 2, "C": 1 << 10, "B": 1 << 20, **far, **one_seed}, f"{fn}: too many elements"),
    ]
ROWS += [
    R(FWD, _F, {"bias": None}, {"x": None}, f"{FWD}: null pointer"),
    R(FWD, _F, None, {"y": None}, f"{FWD}: null pointer"),
    R(BWD, _V, {"amax": None}, {"g_h": None}, f"{BWD}: null pointer"),
    R(BWD, _V, None, {"g_l": None}, f"{BWD}: null pointer"),
    R(BWD, _V, None, {"sexp": None}, f"{BWD}: null pointer"),
    R(BWD, _V, None, {"dx": None}, f"{BWD}: null pointer"),
    R(BWD, _V, {"S": 1}, {"S": 0}, f"{BWD}: extent out of range"),
    R(BWD, _V, {**ONE, "S": I31, "B": 1, "dx": 1 << 62}, {**ONE, "S": 1 << 31, "B": 1, "dx": 1 << 62}, f"{BWD}: extent out of range"),
    # S * B < 2^31
    R(BWD, _V, {**ONE, "S": 1 << 16, "B": (1 << 15) - 1, "dx": 1 << 62}, {**ONE, "S": 1 << 16, "B": 1 << 15, "dx": 1 << 62},
      f"{BWD}: extent out of range"),
    # dx must overlap neither plane.  The planes at the probe's buffer and dx 4096 bytes on: the same address; 2048 halves of a
    # plane fit exactly, one more image does not.  dx at the buffer and the planes 4096 bytes on: 1024 floats of dx fit exactly,
    # one more channel does not.  One plane far away: the other one alone is refused.
    R(BWD, _V, {"S": 3}, {"dx": "same"}, f"{BWD}: dx overlaps g"),
    R(BWD, _V, {"S": 1, "B": 4, "C": 8}, {"S": 1, "B": 5, "C": 8}, f"{BWD}: dx overlaps g"),
    R(BWD, _V, {"g_h": "other", "g_l": "other", "dx": "same", "S": 1, "B": 1, "C": 16},
      {"g_h": "other", "g_l": "other", "dx": "same", "S": 1, "B": 1, "C": 17}, f"{BWD}: dx overlaps g"),
    R(BWD, _V, {"g_h": 1 << 61}, {"g_h": 1 << 61, "dx": "same"}, f"{BWD}: dx overlaps g"),
    R(BWD, _V, {"g_l": 1 << 61}, {"g_l": 1 << 61, "dx": "same"}, f"{BWD}: dx overlaps g"),
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
        if {**row["base"], **row["accept"]}["B"] == 0:
            assert rc == LK_OK  # (an empty batch returns before any HIP call)


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_dwconv.hip")).read()
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
    """every LK_REQUIRE of lk_dwconv.hip: a row's first-refused call came back with that guard's message - the guards of the shared
    checker (their literal starts with "%s: ") under the name of EITHER entry point"""
    messages = _guard_messages()
    assert len(messages) >= 9, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = []
    for msg in messages:
        want += [fn + msg[2:] for fn in (FWD, BWD)] if msg.startswith("%s: ") else [msg]
    assert all(m.startswith((FWD + ": ", BWD + ": ")) for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_dwconv.hip")).read()
    for fn, checker in ((FWD, "dwconv_check_fwd("), (BWD, "dwconv_check_bwd(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FWD, BWD, "lk_dwconv_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_points_refuse():
    """lk_dwconv_variant is host code: every numeric row of the backward's table, asked in this process - a dict on the accepted
    side, None on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    names = ("S", "B", "H", "W", "C", "kh", "kw", "sh", "sw", "ph", "pw")
    for row in ROWS:
        if row["fn"] != BWD or any(f in row["fragment"] for f in ("null pointer", "overlaps")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            r = K.lib.lk_dwconv_variant(*[int(a[n]) for n in names], 1)
            assert (r >= 0) == want, (side, row[side], r)
            asked += 1
    assert asked >= 50
    assert K.dwconv_variant(9, 128, 32, 32, 64, 3, 2, 1) == {"vec": True, "strided": True, "seed_split": False, "tap_class": 0,
                                                              "seeds_per_pass": 4, "seeds_per_slice": 9}
    assert K.dwconv_variant(9, 128, 2, 2, 1024, 5, 1, 2, aligned=False) == {
        "vec": False, "strided": False, "seed_split": False, "tap_class": 1, "seeds_per_pass": 4, "seeds_per_slice": 9}
    assert K.dwconv_variant(9, 2, 2, 2, 64, 3, 1, 1)["seed_split"] and K.dwconv_variant(9, 2, 2, 2, 64, 3, 1, 1)["seeds_per_slice"] == 1
    assert K.dwconv_variant(9, 128, 32, 32, 64, 7, 1, 3) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
