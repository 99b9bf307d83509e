"""The argument contracts of lk_attn_fwd_strided_f32 and lk_attn_vjp_strided_f32 (csrc/lk_attn.hip, csrc/lk_attn_strided.h), probed
at their edges WITHOUT a device - the method and the helpers of tests/test_capi_contracts_attn.py: a table of last-accepted /
first-refused values, a child process that sees no device, and a completeness check of its own.

The strided entry points share the checkers of the layout-1 ones (shape, pointers, scale, overlap of an output with an input,
workspace) and add those of lk_attn_strided.h: the row strides, the element counts they imply, and the three cotangents, which
may interleave in one buffer but may share no element.  The extents that the overlap guard compares run from the first to the
last element of a strided tensor.
"""
import json
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, header_prototypes  # noqa: E402
from tests.test_capi_contracts_attn import SENTINEL, _AttnProbe  # noqa: E402

FWD, VJP = "lk_attn_fwd_strided_f32", "lk_attn_vjp_strided_f32"
HD, LD = 24, 72  # H * D and the row stride of a packed [.., 3 H D] projection
_F = dict(B=2, H=3, T=5, D=8, ldq=LD, scale=0.5, causal=0)
_V = dict(S=3, **_F, ldd=LD, ws_bytes=368)  # delta: 4 * 3 * 2 * 3 * 5 = 360 bytes, rounded up to 16
N1, NS, NL = 2 * 3 * 5 * 8 * 4, 3 * 2 * 3 * 5 * 8 * 4, 2 * 3 * 5 * 4  # o, go, lse
NI, ND = (9 * LD + HD) * 4, (29 * LD + HD) * 4  # first to last element of q / k / v (10 rows) and of dq / dk / dv (30 rows)
ONE = dict(B=1, H=1, T=1, D=4, ldq=4)
ONE_V = dict(S=1, **ONE, ldd=4, ws_bytes=1 << 40)
BIG = {"ws_bytes": 1 << 40}

ROWS = []
for fn, base, ptrs in ((FWD, _F, ("q", "k", "v", "o", "lse")), (VJP, _V, ("go", "q", "k", "v", "o", "lse", "dq", "dk", "dv", "ws"))):
    one = ONE if fn == FWD else ONE_V
    big = {} if fn == FWD else BIG
    ROWS += [R(fn, base, None, {p: None}, f"{fn}: null pointer") for p in ptrs]
    ROWS += [R(fn, base, None, {p: "odd"}, f"{fn}: pointers must be 16-byte aligned") for p in (ptrs[0], ptrs[-1])]
    ROWS += [
        # the layout-1 contract, through the same checkers (the layout itself is no argument here)
        R(fn, base, {"D": 4}, {"D": 0}, f"{fn}: head dim out of range"),
        R(fn, base, {**one, "D": 128, "ldq": 128, **({"ldd": 128} if fn == VJP else {})},
          {**one, "D": 132, "ldq": 132, **({"ldd": 132} if fn == VJP else {})}, f"{fn}: head dim out of range"),
        R(fn, base, {"T": 1}, {"T": 0}, f"{fn}: extent out of range"),
        R(fn, base, {"B": 0}, {"B": -1}, f"{fn}: extent out of range"),
        R(fn, base, {**one, "H": (1 << 16) - 1, "ldq": (1 << 18) - 4, **({"ldd": (1 << 18) - 4} if fn == VJP else {})},
          {**one, "H": 1 << 16, "ldq": 1 << 18, **({"ldd": 1 << 18} if fn == VJP else {})}, f"{fn}: extent out of range"),
        R(fn, base, {**one, "B": (1 << 20) - 1, "T": 1 << 14, "D": 64, "ldq": 64, **({"ldd": 64} if fn == VJP else {}), **big},
          {**one, "B": 1 << 20, "T": 1 << 14, "D": 64, "ldq": 64, **({"ldd": 64} if fn == VJP else {}), **big}, f"{fn}: too many elements (S"),
        R(fn, base, {**one, "B": 1 << 16, "H": (1 << 15) - 1, "ldq": 1 << 17, **({"ldd": 1 << 17} if fn == VJP else {}), **big},
          {**one, "B": 1 << 16, "H": 1 << 15, "ldq": 1 << 17, **({"ldd": 1 << 17} if fn == VJP else {}), **big}, f"{fn}: too many row blocks"),
        R(fn, base, {"scale": -3.0e38}, {"scale": math.inf}, f"{fn}: scale must be finite"),
        R(fn, base, {"scale": 0.0}, {"scale": math.nan}, f"{fn}: scale must be finite"),
        # the row stride of the operands: at least H D, a multiple of 4
        R(fn, base, {"ldq": HD}, {"ldq": HD - 4}, f"{fn}: row stride out of range"),
        R(fn, base, {"ldq": HD + 4}, {"ldq": HD + 2}, f"{fn}: row stride out of range"),
        R(fn, base, {"ldq": LD + 8}, {"ldq": -LD}, f"{fn}: row stride out of range"),
        # B T ldq < 2^40: 2^10 rows
        R(fn, base, {**one, "B": 1 << 10, "ldq": (1 << 30) - 4, **big}, {**one, "B": 1 << 10, "ldq": 1 << 30, **big},
          f"{fn}: too many elements (B * T * ldq"),
    ]
ROWS += [
    R(VJP, _V, {"S": 1}, {"S": 0}, f"{VJP}: extent out of range"),
    R(VJP, _V, {"ldd": HD}, {"ldd": HD - 4}, f"{VJP}: row stride out of range"),
    R(VJP, _V, {"ldd": HD + 4}, {"ldd": HD + 2}, f"{VJP}: row stride out of range"),
    R(VJP, _V, {"ldd": LD + 12}, {"ldd": 0}, f"{VJP}: row stride out of range"),
    # S B T ldd < 2^40: 2^10 rows
    R(VJP, _V, {**ONE_V, "S": 1 << 4, "B": 1 << 6, "ldd": (1 << 30) - 4}, {**ONE_V, "S": 1 << 4, "B": 1 << 6, "ldd": 1 << 30},
      f"{VJP}: too many elements (B * T * ldq"),
    # no output may overlap an input; a strided tensor's extent runs from its first to its last element
    R(FWD, _F, {"o": ("at", "q", NI)}, {"o": ("at", "q", NI - 16)}, f"{FWD}: an output overlaps an input"),
    R(FWD, _F, {"o": ("at", "k", -N1)}, {"o": ("at", "k", -N1 + 16)}, f"{FWD}: an output overlaps an input"),
    R(FWD, _F, {"lse": ("at", "v", NI)}, {"lse": ("at", "v", NI - 16)}, f"{FWD}: an output overlaps an input"),
    R(VJP, _V, {"dq": ("at", "go", NS)}, {"dq": ("at", "go", NS - 16)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"dk": ("at", "q", -ND)}, {"dk": ("at", "q", -ND + 16)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"dv": ("at", "v", NI)}, {"dv": ("at", "v", NI - 16)}, f"{VJP}: an output overlaps an input"),
    # (between the rows of an input is inside its extent)
    R(VJP, _V, {"dq": ("at", "lse", NL + 8)}, {"dq": ("at", "q", HD * 4)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"ws": ("at", "o", -368)}, {"ws": ("at", "o", -352)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"ws_bytes": 368}, {"ws_bytes": 367}, f"{VJP}: workspace too small"),
    # dq, dk, dv may interleave in one buffer - rows of H D floats, ldd apart - but share no element
    R(VJP, _V, {"dk": ("at", "dq", HD * 4), "dv": ("at", "dq", 2 * HD * 4)}, {"dk": ("at", "dq", HD * 4 - 16)},
      f"{VJP}: the outputs overlap each other"),
    R(VJP, _V, {"dv": ("at", "dq", (LD - HD) * 4)}, {"dv": ("at", "dq", (LD - HD) * 4 + 16)}, f"{VJP}: the outputs overlap each other"),
    R(VJP, _V, {"dk": ("at", "dq", -HD * 4)}, {"dk": ("at", "dq", -HD * 4 + 16)}, f"{VJP}: the outputs overlap each other"),
    R(VJP, _V, {"dk": ("at", "dq", ND)}, {"dk": ("at", "dq", 0)}, f"{VJP}: the outputs overlap each other"),
    R(VJP, _V, {"dv": ("at", "dk", -ND)}, {"dv": ("at", "dk", LD * 4)}, f"{VJP}: the outputs overlap each other"),
    # (ldd = H D leaves no room between the rows: apart by the whole extent or not at all)
    R(VJP, _V, {"ldd": HD, "dk": ("at", "dq", 30 * HD * 4)}, {"ldd": HD, "dk": ("at", "dq", 30 * HD * 4 - 16)},
      f"{VJP}: the outputs overlap each other"),
]


def _child_main():
    import torch

    def emit(obj):
        sys.stdout.write(json.dumps(obj) + "\n")
        sys.stdout.flush()

    if torch.cuda.device_count() != 0:
        emit({"fatal": "device visible"})
        return 3
    P = _AttnProbe()
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
            assert rc == LK_OK  # (nothing to write: returns before any HIP call)


def test_an_empty_batch_returns_ok_before_any_hip_call():
    P = _AttnProbe()
    assert P.call(FWD, {**_F, "B": 0})[0] == LK_OK
    assert P.call(VJP, {**_V, "B": 0, "ws_bytes": 0})[0] == LK_OK


def _guard_messages(fname):
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", fname)).read()
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for m in re.finditer(r"LK_REQUIRE\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', text[m.end():j])))
    return out


def test_every_guard_is_reached_by_a_row_of_both_entry_points(probes):
    """every LK_REQUIRE of lk_attn.hip and of lk_attn_strided.h: a row's first-refused call came back with that guard's message
    under the strided entry point's name - for both, except the guards of arguments that the forward does not have (the layout,
    the workspace, the cotangents)"""
    shared, own = _guard_messages("lk_attn.hip"), _guard_messages("lk_attn_strided.h")
    assert len(shared) >= 9 and len(own) == 3 and all(m.startswith("%s: ") for m in shared + own), (shared, own)
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    missing = []
    for m in shared + own:
        if "layout is" in m:
            continue  # (the strided entry points have no layout argument: they pass 1)
        for fn in (FWD, VJP):
            if fn == FWD and ("workspace" in m or "outputs overlap each other" in m):
                continue
            if fn + m[2:].replace("%%", "%") not in refused:
                missing.append((fn, m))
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """no guard in an extern "C" body; the shape, then the strides, then the pointers, before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_attn.hip")).read()
    for fn in (FWD, VJP):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index("attn_check_shape(") < body.index("attn_check_strides(") < body.index("attn_check(") < body.index("hipStream_t")
    body = text[text.index(f'extern "C" int {VJP}'):]
    assert body.index("attn_check_interleave(") < body.index("hipStream_t")


def test_the_path_is_what_the_layout_1_variant_names():
    """no variant query of their own: the plan is that of ``lk_attn_variant(S, B, H, T, D, 1, causal)``, whatever the strides"""
    from laplace_amd._lib import HipKernels

    assert HipKernels().attn_variant(9, 128, 3, 64, 64, 1, False) == {"resident": True, "seed_split": True, "dp": 64, "causal": False,
                                                                     "layout": 1, "seeds_per_slice": 5, "owner_blocks": 1}
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_attn.hip")).read()
    for fn in (FWD, VJP):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert re.search(r"attn_check_shape\(fn, \w+, B, H, T, D, 1, &p\)", body)
        assert set(re.findall(r"p\.(\w+)\.(\w+) =", body)) <= {("in", "row"), ("in", "batch"), ("out", "row"), ("out", "batch"), ("out", "seed")}


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
