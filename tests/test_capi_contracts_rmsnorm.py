"""The argument contracts of lk_rmsnorm_fwd_f32, lk_rmsnorm_vjp_f32 and lk_rmsnorm_variant (csrc/lk_rmsnorm.hip), probed at their
edges WITHOUT a device - the method of tests/test_capi_contracts.py (whose helpers are reused) and
tests/test_capi_contracts_normvjp.py: a table of last-accepted / first-refused values, a child process that sees no device, and a
completeness check of its own.

lk_rmsnorm.hip keeps every argument check in checker functions that the entry points call before the first HIP call (the shape
guards both entry points share are one macro, expanded under either name).  Without a device a call that passes its checker ends
in LK_ELAUNCH, or in LK_OK for an empty matrix.  lk_rmsnorm_variant is host only: a path word >= 0, or a negative value for
exactly the shapes the entry points refuse.
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

FWD, VJP, VARIANT = "lk_rmsnorm_fwd_f32", "lk_rmsnorm_vjp_f32", "lk_rmsnorm_variant"
_F = dict(w=None, rows=4, D=30, eps=1e-6)
# (g and dx: two places of the probe's buffer, 4096 bytes apart; S * rows * D * 4 = 1440 bytes)
_V = dict(g="same", dx="other", w=None, amax=None, S=3, rows=4, D=30)
I31, I30 = (1 << 31) - 1, (1 << 30) - 1
ROWS = []
for fn, base in ((FWD, _F), (VJP, _V)):
    out = "y" if fn == FWD else "dx"
    # one seed, and dx at an address far from g: nothing is touched without a device, and the overlap guard must not be the one
    # that answers a probe of the extents
    big = {"S": 1, "dx": 1 << 62} if fn == VJP else {}
    ROWS += [
        R(fn, base, None, {"x": None}, f"{fn}: null pointer"),
        R(fn, base, None, {"rstd": None}, f"{fn}: null pointer"),
        R(fn, base, None, {out: None}, f"{fn}: null pointer"),
        R(fn, base, {"rows": 0}, {"rows": -1}, f"{fn}: extent out of range"),
        R(fn, base, {"D": 1}, {"D": 0}, f"{fn}: extent out of range"),
        R(fn, base, {"rows": I31, "D": 1, **big}, {"rows": 1 << 31, "D": 1, **big}, f"{fn}: extent out of range"),
        R(fn, base, {"D": I30, "rows": 1, **big}, {"D": 1 << 30, "rows": 1, **big}, f"{fn}: extent out of range"),
        # S * rows * D < 2^40: 2^10 rows of 2^30 - 1 pass, 2^11 rows of 2^29 do not
        R(fn, base, {"rows": 1 << 10, "D": I30, **big}, {"rows": 1 << 11, "D": 1 << 29, **big}, f"{fn}: too many elements"),
    ]
ROWS += [
    R(VJP, _V, None, {"g": None}, f"{VJP}: null pointer"),
    R(VJP, _V, {"S": 1}, {"S": 0}, f"{VJP}: extent out of range"),
    R(VJP, _V, {"S": I31, "rows": 0}, {"S": 1 << 31, "rows": 0}, f"{VJP}: extent out of range"),
    # ... with the seeds in the product
    R(VJP, _V, {"S": 1 << 10, "rows": 1 << 10, "D": (1 << 20) - 1, "dx": 1 << 62}, {"S": 1 << 10, "rows": 1 << 10, "D": 1 << 20, "dx": 1 << 62},
      f"{VJP}: too many elements"),
    # dx must not overlap g (g at the probe's buffer, dx 4096 bytes on): the same address; one float inside where 4096 bytes fit
    # exactly; 1024 floats fit exactly, one more row does not
    R(VJP, _V, {"S": 3}, {"dx": "same"}, f"{VJP}: dx overlaps g"),
    R(VJP, _V, {"S": 8, "rows": 16, "D": 8}, {"S": 8, "rows": 16, "D": 8, "dx": "odd"}, f"{VJP}: dx overlaps g"),
    R(VJP, _V, {"S": 1, "rows": 16, "D": 64}, {"S": 1, "rows": 17, "D": 64}, f"{VJP}: dx overlaps g"),
]
# lk_rmsnorm_variant: (accepted, refused) shapes at the same edges
VARIANT_EDGES = [
    (dict(S=1, rows=0, D=1), dict(S=0, rows=0, D=1)), (dict(S=I31, rows=0, D=1), dict(S=1 << 31, rows=0, D=1)),
    (dict(S=1, rows=0, D=1), dict(S=1, rows=-1, D=1)), (dict(S=1, rows=I31, D=1), dict(S=1, rows=1 << 31, D=1)),
    (dict(S=1, rows=1, D=1), dict(S=1, rows=1, D=0)), (dict(S=1, rows=1, D=I30), dict(S=1, rows=1, D=1 << 30)),
    (dict(S=1 << 10, rows=1 << 10, D=(1 << 20) - 1), dict(S=1 << 10, rows=1 << 10, D=1 << 20)),
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
    for i, pair in enumerate(VARIANT_EDGES):
        for side, shape in zip(("accept", "refuse"), pair):
            for aligned in (0, 1):
                rc, _ = P.call(VARIANT, {**shape, "aligned": aligned})
                emit({"variant": i, "side": side, "aligned": aligned, "rc": rc})
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
        elif "variant" in obj:
            rows[("variant", obj["variant"], obj["side"], obj["aligned"])] = obj["rc"]
        elif "done" in obj:
            done = True
    if proc.returncode != 0 or not done:
        pytest.fail(f"the probing child ended with status {proc.returncode}; last probe started: {last}\n" + proc.stderr[-2000:])
    return rows


def _row_id(i):
    return (ROWS[i]["fn"][11:14] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items()))[:100]


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")
    assert {p[2] for p in protos[VARIANT]} == {"S", "rows", "D", "aligned"}


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
        if {**row["base"], **row["accept"]}["rows"] == 0:
            assert rc == LK_OK  # (an empty matrix returns before any HIP call)


@pytest.mark.parametrize("i", range(len(VARIANT_EDGES)))
def test_the_variant_refuses_exactly_what_the_entry_points_refuse(probes, i):
    for aligned in (0, 1):
        assert probes[("variant", i, "accept", aligned)] >= 0, VARIANT_EDGES[i][0]
        assert probes[("variant", i, "refuse", aligned)] < 0, VARIANT_EDGES[i][1]


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_rmsnorm.hip")).read()
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
    """every LK_REQUIRE of lk_rmsnorm.hip: a row's first-refused call came back with that guard's message - the guards of the
    shared macro (their literal starts with ": ") under the name of EITHER entry point"""
    messages = _guard_messages()
    assert len(messages) == 5, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    want = []
    for msg in messages:
        want += [fn + msg for fn in (FWD, VJP)] if msg.startswith(": ") else [msg]
    assert all(m.startswith((FWD + ": ", VJP + ": ")) for m in want), want
    missing = [m for m in want if m not in refused]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_their_checkers_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body, the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_rmsnorm.hip")).read()
    for fn, checker in ((FWD, "rmsnorm_check_fwd("), (VJP, "rmsnorm_check_vjp(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index(checker) < body.index("hipLaunchKernelGGL")


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
