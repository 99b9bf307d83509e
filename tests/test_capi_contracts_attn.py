"""The argument contracts of lk_attn_fwd_f32, lk_attn_vjp_f32, lk_attn_vjp_workspace_bytes and lk_attn_variant (csrc/lk_attn.hip),
probed at their edges WITHOUT a device - the method of tests/test_capi_contracts_normtap.py (whose helpers are reused): a table of
last-accepted / first-refused values, a child process that sees no device, and a completeness check of its own.

lk_attn.hip keeps every argument check in checker functions that the entry points call before the first HIP call.  Without a
device a call that passes them ends in LK_ELAUNCH, or in LK_OK for an empty batch.  No pointer is ever read on the host, so the
probe hands every pointer parameter an address of its own, 2^44 bytes from the next one (the overlap guard compares extents of up
to 2^42 bytes); ``("at", name, bytes)`` places a pointer relative to another parameter's.
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

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, _Probe, header_prototypes  # noqa: E402

FWD, VJP = "lk_attn_fwd_f32", "lk_attn_vjp_f32"
_F = dict(B=2, H=3, T=5, D=8, layout=0, scale=0.5, causal=0)
_V = dict(S=3, **_F, ws_bytes=368)  # delta: 4 * 3 * 2 * 3 * 5 = 360 bytes, rounded up to 16
N1, NS, NL = 2 * 3 * 5 * 8 * 4, 3 * 2 * 3 * 5 * 8 * 4, 2 * 3 * 5 * 4
ONE = dict(B=1, H=1, T=1, D=4)  # one row: the count guard stays out of an extent's way
ONE_V = dict(S=1, **ONE, ws_bytes=1 << 40)
I31 = (1 << 31) - 1

ROWS = []
for fn, base, ptrs in ((FWD, _F, ("q", "k", "v", "o", "lse")), (VJP, _V, ("go", "q", "k", "v", "o", "lse", "dq", "dk", "dv", "ws"))):
    one = ONE if fn == FWD else ONE_V
    ROWS += [R(fn, base, None, {p: None}, f"{fn}: null pointer") for p in ptrs]
    ROWS += [R(fn, base, None, {p: "odd"}, f"{fn}: pointers must be 16-byte aligned") for p in (ptrs[0], ptrs[-1])]
    ROWS += [
        R(fn, base, {"layout": 1}, {"layout": 2}, f"{fn}: layout is 0"),
        R(fn, base, {"layout": 0}, {"layout": -1}, f"{fn}: layout is 0"),
        R(fn, base, {"D": 4}, {"D": 0}, f"{fn}: head dim out of range"),
        R(fn, base, {"D": 128}, {"D": 132}, f"{fn}: head dim out of range"),
        R(fn, base, {"D": 12}, {"D": 10}, f"{fn}: head dim out of range"),
        R(fn, base, {"T": 1}, {"T": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**one, "T": (1 << 15) - 1}, {**one, "T": 1 << 15}, f"{fn}: extent out of range"),
        R(fn, base, {"B": 0}, {"B": -1}, f"{fn}: extent out of range"),
        R(fn, base, {"H": 1}, {"H": 0}, f"{fn}: extent out of range"),
        R(fn, base, {**one, "H": (1 << 16) - 1}, {**one, "H": 1 << 16}, f"{fn}: extent out of range"),
        # S * B * H * T * D < 2^40: 2^14 positions x 64 = 2^20 elements per sample (2^8 row blocks)
        R(fn, base, {**one, "B": (1 << 20) - 1, "T": 1 << 14, "D": 64, **({"ws_bytes": 1 << 40} if fn == VJP else {})},
          {**one, "B": 1 << 20, "T": 1 << 14, "D": 64, **({"ws_bytes": 1 << 40} if fn == VJP else {})},
          f"{fn}: too many elements"),
        # B * H * ceil(T / 64) < 2^31 at T = 1
        R(fn, base, {**one, "B": 1 << 16, "H": (1 << 15) - 1, **({"ws_bytes": 1 << 40} if fn == VJP else {})},
          {**one, "B": 1 << 16, "H": 1 << 15, **({"ws_bytes": 1 << 40} if fn == VJP else {})}, f"{fn}: too many row blocks"),
        R(fn, base, {"scale": -3.0e38}, {"scale": math.inf}, f"{fn}: scale must be finite"),
        R(fn, base, {"scale": 0.0}, {"scale": math.nan}, f"{fn}: scale must be finite"),
    ]
ROWS += [
    R(FWD, _F, {**ONE, "B": I31}, {**ONE, "B": 1 << 31}, f"{FWD}: extent out of range"),
    R(VJP, _V, {"S": 1, "ws_bytes": 368}, {"S": 0}, f"{VJP}: extent out of range"),
    R(VJP, _V, {**ONE_V, "S": 1 << 16, "B": (1 << 15) - 1, "ws_bytes": 1 << 40}, {**ONE_V, "S": 1 << 16, "B": 1 << 15, "ws_bytes": 1 << 40},
      f"{VJP}: extent out of range"),
    # no output may overlap an input: an output that ends where an input begins is the last accepted placement
    R(FWD, _F, {"o": ("at", "q", N1)}, {"o": ("at", "q", N1 - 16)}, f"{FWD}: an output overlaps an input"),
    R(FWD, _F, {"o": ("at", "k", -N1)}, {"o": ("at", "k", -N1 + 16)}, f"{FWD}: an output overlaps an input"),
    R(FWD, _F, {"lse": ("at", "v", -NL - 8)}, {"lse": ("at", "v", -NL + 8)}, f"{FWD}: an output overlaps an input"),
    R(VJP, _V, {"dq": ("at", "go", NS)}, {"dq": ("at", "go", NS - 16)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"dk": ("at", "q", N1)}, {"dk": ("at", "q", 0)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"dv": ("at", "lse", -NS)}, {"dv": ("at", "lse", -NS + 16)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"ws": ("at", "o", -368)}, {"ws": ("at", "o", -352)}, f"{VJP}: an output overlaps an input"),
    R(VJP, _V, {"ws_bytes": 368}, {"ws_bytes": 367}, f"{VJP}: workspace too small"),
]

SENTINEL = ("lk_symmetrize_f32", {"n": -1})


class _AttnProbe(_Probe):
    """every pointer parameter at an address of its own (never read: host checks only, no device)"""

    def args(self, fn, values):
        protos = self.protos[fn]
        home = {pname: (1 << 50) + i * (1 << 44) for i, (kind, _, pname) in enumerate(protos) if kind == "ptr"}
        out, left = [], dict(values)
        for kind, ctype, pname in protos:
            v = left.pop(pname, "__default__")
            if kind == "ptr":
                if pname == "stream" or v is None:
                    v = None
                elif v == "__default__":
                    v = home[pname]
                elif v == "odd":
                    v = home[pname] + 4
                else:
                    assert v[0] == "at"
                    v = home[v[1]] + int(v[2])
                out.append(v)
            else:
                if isinstance(v, str):
                    raise KeyError(f"{fn}: no value for {pname}")
                out.append(v)
        if left:
            raise KeyError(f"{fn}: unknown parameters {sorted(left)}")
        return out


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


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_attn.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for m in re.finditer(r"LK_REQUIRE\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', text[m.end():j])))
    return out


def test_every_guard_of_the_file_is_reached_by_a_row_of_both_entry_points(probes):
    """every LK_REQUIRE of lk_attn.hip (their literals start with "%s: "): a row's first-refused call came back with that guard's
    message under the entry point's name - for both entry points, except the workspace guard, which is the VJP's alone"""
    messages = _guard_messages()
    assert len(messages) >= 9 and all(m.startswith("%s: ") for m in messages), messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    missing = []
    for m in messages:
        for fn in (FWD, VJP):
            if fn == FWD and "workspace" in m:
                continue
            if fn + m[2:].replace("%%", "%") not in refused:
                missing.append((fn, m))
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checkers before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_attn.hip")).read()
    for fn in (FWD, VJP):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index("attn_check_shape(") < body.index("attn_check(") < body.index("hipStream_t")
    from tests.test_capi_contracts import guarded_entry_points

    assert not {FWD, VJP, "lk_attn_variant", "lk_attn_vjp_workspace_bytes"} & guarded_entry_points()


def test_the_host_queries_refuse_what_the_entry_points_refuse():
    """lk_attn_variant and lk_attn_vjp_workspace_bytes are host code: every row of the table that is about the shape, asked in
    this process - a plan and a size on the accepted side, a negative value and 0 on the refused one"""
    from laplace_amd._lib import HipKernels

    K, asked = HipKernels(), 0
    for row in ROWS:
        if not any(f in row["fragment"] for f in ("extent out of range", "too many", "head dim", "layout is")):
            continue
        for side, want in (("accept", True), ("refuse", False)):
            if row[side] is None:
                continue
            a = {"S": 1, **row["base"], **row[side]}
            dims = [int(a[n]) for n in ("S", "B", "H", "T", "D")]
            r = K.lib.lk_attn_variant(*dims, int(a["layout"]), int(a["causal"]))
            assert (r >= 0) == want, (side, row[side], r)
            if "layout" not in row["fragment"]:
                nbytes = K.lib.lk_attn_vjp_workspace_bytes(*dims)
                assert (nbytes > 0 or dims[1] == 0) == want and (not want or nbytes >= 4 * dims[0] * dims[1] * dims[2] * dims[3])
            asked += 1
    assert asked >= 40
    assert K.attn_variant(9, 128, 3, 64, 64, 1, False) == {"resident": True, "seed_split": True, "dp": 64, "causal": False,
                                                           "layout": 1, "seeds_per_slice": 5, "owner_blocks": 1}
    assert K.attn_variant(1, 32, 12, 128, 64) == {"resident": True, "seed_split": False, "dp": 64, "causal": False, "layout": 0,
                                                  "seeds_per_slice": 1, "owner_blocks": 2}
    assert K.attn_variant(2, 1, 1, 257, 8, 0, True)["resident"] is False
    assert K.attn_variant(9, 128, 3, 64, 6) is None


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
