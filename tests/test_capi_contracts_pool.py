"""The argument contracts of lk_pool_fwd_nhwc_f32, lk_pool_vjp_nhwc_f32 and lk_pool_variant (csrc/lk_pool.hip), probed at their
edges WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and
tests/test_capi_contracts_normvjp.py: a table of last-accepted / first-refused values, a child process that sees no device, and
a completeness check of its own.

lk_pool.hip keeps every argument check in checker functions that the entry points call before the first HIP call (the shape
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

FWD, VJP = "lk_pool_fwd_nhwc_f32", "lk_pool_vjp_nhwc_f32"
_GEO = dict(kind=0, B=2, H=8, W=8, C=4, kh=2, kw=2, sh=2, sw=2, ph=0, pw=0, count_include_pad=1, divisor_override=0)
_F = dict(_GEO)
# (g and dx: two places of the probe's buffer, 4096 bytes apart; g is 3 * 2 * 4 * 4 * 4 floats = 1536 bytes)
_V = dict(_GEO, g="same", dx="other", amax=None, S=3)
I31, I30 = (1 << 31) - 1, (1 << 30) - 1
ONE = dict(H=1, W=1, C=1, kh=1, kw=1, sh=1, sw=1)  # one pixel, one channel: the count guard stays out of an extent's way
ROWS = []
for fn, base in ((FWD, _F), (VJP, _V)):
    out = "y" if fn == FWD else "dx"
    # dx at an address far from g: nothing is touched without a device, and the overlap guard must not answer a probe of the extents
    far = {"dx": 1 << 62} if fn == VJP else {}
    ROWS += [
        R(fn, base, None, {out: None}, f"{fn}: null pointer"),
        R(fn, base, {"kind": 1, "arg": None}, {"kind": 2}, f"{fn}: kind must be LK_POOL_MAX (0) or LK_POOL_AVG (1)"),
        R(fn, base, {"kind": 0}, {"kind": -1}, f"{fn}: kind must be"),
        R(fn, base, {"kh": 8}, {"kh": 9, "H": 16}, f"{fn}: window out of range"),
        R(fn, base, {"kw": 8}, {"kw": 9, "W": 16}, f"{fn}: window out of range"),
        R(fn, base, {"kh": 1}, {"kh": 0}, f"{fn}: window out of range"),
        R(fn, base, {"kw": 1}, {"kw": 0}, f"{fn}: window out of range"),
        R(fn, base, {"sh": 1}, {"sh": 0}, f"{fn}: stride out of range"),
        R(fn, base, {"sw": 1}, {"sw": 0}, f"{fn}: stride out of range"),
        R(fn, base, {"sh": 32767}, {"sh": 32768}, f"{fn}: stride out of range"),
        R(fn, base, {"sw": 32767}, {"sw": 32768}, f"{fn}: stride out of range"),
        # padding at most half the window, rounded down: 2 of 4 and 2 of 5, never 3
        R(fn, base, {"kh": 4, "ph": 2}, {"kh": 4, "ph": 3}, f"{fn}: padding out of range"),
        R(fn, base, {"kh": 5, "ph": 2}, {"kh": 5, "ph": 3}, f"{fn}: padding out of range"),
        R(fn, base, {"kw": 4, "pw": 2}, {"kw": 4, "pw": 3}, f"{fn}: padding out of range"),
        R(fn, base, {"kw": 3, "pw": 1}, {"kw": 3, "pw": 2}, f"{fn}: padding out of range"),
        R(fn, base, {"ph": 0}, {"ph": -1}, f"{fn}: padding out of range"),
        R(fn, base, {"pw": 0}, {"pw": -1}, f"{fn}: padding out of range"),
        R(fn, base, {"B": 0}, {"B": -1}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "H": 32767, **far}, {**ONE, "H": 32768, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "W": 32767, **far}, {**ONE, "W": 32768, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "H": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "W": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE}, {**ONE, "C": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "C": I30, "B": 1, **far}, {**ONE, "C": 1 << 30, "B": 1, **far}, f"{fn}: extent out of range"),
        R(fn, base, {**ONE, "B": I31, **far, **({"S": 1} if fn == VJP else {})},
          {**ONE, "B": 1 << 31, **far, **({"S": 1} if fn == VJP else {})}, f"{fn}: extent out of range"),
        # OH = (H + 2 ph - kh) / sh + 1 >= 1: a two-row window on one row without padding has no output
        R(fn, base, {"H": 2}, {"H": 1}, f"{fn}: empty output"),
        R(fn, base, {"W": 2}, {"W": 1}, f"{fn}: empty output"),
        R(fn, base, {"H": 1, "ph": 1}, {"H": 1, "kh": 4, "ph": 1}, f"{fn}: empty output"),
        # S * B * C * max(H * W, OH * OW) < 2^40: 2^10 pixels x 2^10 channels x 2^20 images; with a window of 2, stride 1 and
        # padding 1 it is the OUTPUT that has 2^10 pixels (the input has 31 x 31)
        R(fn, base, {"H": 32, "W": 32, "C": 1 << 10, "B": (1 << 20) - 1, **far, **({"S": 1} if fn == VJP else {})},
          {"H": 32, "W": 32, "C": 1 << 10, "B": 1 << 20, **far, **({"S": 1} if fn == VJP else {})}, f"{fn}: too many elements"),
        R(fn, base, {"H": 31, "W": 31, "sh": 1, "sw": 1, "ph": 1, "pw": 1, "C": 1 << 10, "B": (1 << 20) - 1, **far,
                     **({"S": 1} if fn == VJP else {})},
          {"H": 31, "W": 31, "sh": 1, "sw": 1, "ph": 1, "pw": 1, "C": 1 << 10, "B": 1 << 20, **far,
           **({"S": 1} if fn == VJP else {})}, f"{fn}: too many elements"),
        R(fn, base, {"kind": 0}, {"kind": 0, "arg": None}, f"{fn}: arg must be given for LK_POOL_MAX and null for LK_POOL_AVG"),
        R(fn, base, {"kind": 1, "arg": None}, {"kind": 1}, f"{fn}: arg must be given for LK_POOL_MAX and null for LK_POOL_AVG"),
    ]
ROWS += [
    R(FWD, _F, None, {"x": None}, f"{FWD}: null pointer"),
    R(VJP, _V, None, {"g": None}, f"{VJP}: null pointer"),
    R(VJP, _V, {"S": 1}, {"S": 0}, f"{VJP}: extent out of range"),
    R(VJP, _V, {**ONE, "S": I31, "B": 1, "dx": 1 << 62}, {**ONE, "S": 1 << 31, "B": 1, "dx": 1 << 62}, f"{VJP}: extent out of range"),
    # S * B < 2^31
    R(VJP, _V, {**ONE, "S": 1 << 16, "B": (1 << 15) - 1, "dx": 1 << 62}, {**ONE, "S": 1 << 16, "B": 1 << 15, "dx": 1 << 62},
      f"{VJP}: extent out of range"),
    # dx must not overlap g.  g at the probe's buffer and dx 4096 bytes on: the same address; 1024 floats of g fit exactly, one
    # more image does not.  dx at the buffer and g 4096 bytes on: 1024 floats of dx fit exactly, one more channel does not.
    R(VJP, _V, {"S": 3}, {"dx": "same"}, f"{VJP}: dx overlaps g"),
    R(VJP, _V, {"S": 1, "B": 4, "C": 16}, {"S": 1, "B": 5, "C": 16}, f"{VJP}: dx overlaps g"),
    R(VJP, _V, {"g": "other", "dx": "same", "S": 1, "B": 1, "C": 16}, {"g": "other", "dx": "same", "S": 1, "B": 1, "C": 17},
      f"{VJP}: dx overlaps g"),
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
    return (ROWS[i]["fn"][8:11] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items()))[:100]


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
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_pool.hip")).read()
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
    """every LK_REQUIRE of lk_pool.hip: a row's first-refused call came back with that guard's message - the guards of the shared
    checker (their literal starts with "%s: ") under the name of EITHER entry point"""
    messages = _guard_messages()
    assert len(messages) >= 11, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = []
    for msg in messages:
        want += [fn + msg[2:] for fn in (FWD, VJP)] if msg.startswith("%s: ") else [msg]
    assert all(m.startswith((FWD + ": ", VJP + ": ")) for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_pool.hip")).read()
    for fn, checker in ((FWD, "pool_check_fwd("), (VJP, "pool_check_vjp(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("hipLaunchKernelGGL")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FWD, VJP, "lk_pool_variant"} & guarded_entry_points()  # (that file's table owes these entry points no row)


def test_the_variant_query_refuses_what_the_entry_points_refuse():
    """lk_pool_variant is host code: every numeric row of the VJP's table, asked in this process - a dict on the accepted side, None
    on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    names = ("kind", "S", "B", "H", "W", "C", "kh", "kw", "sh", "sw", "ph", "pw")
    for row in ROWS:
        if row["fn"] != VJP or any(f in row["fragment"] for f in ("null pointer", "overlaps", "arg must be")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {**row["base"], **row[side]}
            r = K.lib.lk_pool_variant(*[int(a[n]) for n in names], 1)
            assert (r >= 0) == want, (side, row[side], r)
            asked += 1
    assert asked >= 50
    assert K.pool_variant(0, 9, 128, 32, 32, 64, 3, 2, 1) == {"vec": True, "summing": True, "seed_split": False,
                                                               "seeds_per_pass": 4, "seeds_per_slice": 9}
    assert K.pool_variant(1, 9, 128, 32, 32, 64, 9, 2, 1) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
