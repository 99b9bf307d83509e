"""The argument contract of the embedding entry points (csrc/lk_embed.hip), probed at its edges WITHOUT a device - the method
of tests/test_capi_contracts.py (whose helpers are reused), with a table, a child process and a completeness check of its own,
as tests/test_capi_contracts_gconv.py.

lk_embed.hip keeps every argument check in checker functions that the entry points call before the first HIP call; the
completeness test of tests/test_capi_contracts.py reads rows only from its own table and therefore does not see these entry
points.  These rows can be folded into that table.
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

JAC, DIAG, QUAD = "lk_jac_embed_f32", "lk_diag_embed_f32", "lk_diag_quadform_embed_f32"
FNS = (JAC, DIAG, QUAD)
I31 = (1 << 31) - 1
_SHAPE = dict(B=3, T=7, D=4, V=5, padding_idx=-1)
BASE = {JAC: dict(_SHAPE, S=2, P=24, col0=2), DIAG: dict(_SHAPE, S=2, alpha=1.0), QUAD: dict(_SHAPE, C=2)}
SEEDS = {JAC: "S", DIAG: "S", QUAD: "C"}
OUT = {JAC: "Js", DIAG: "h", QUAD: "fvar"}
IDS = {JAC: ("order", "sorted_ids"), DIAG: ("order", "sorted_ids"), QUAD: ("order_row", "sorted_ids_row")}


def _shared(fn):
    """the rows of the contract all three entry points share, for one of them"""
    b, s = BASE[fn], SEEDS[fn]
    wide = {"P": 1 << 40} if fn == JAC else {}
    return [
        R(fn, b, None, {"g": None}, f"{fn}: null pointer"),
        R(fn, b, None, {IDS[fn][0]: None}, f"{fn}: null pointer"),
        R(fn, b, None, {IDS[fn][1]: None}, f"{fn}: null pointer"),
        R(fn, b, None, {OUT[fn]: None}, f"{fn}: null pointer"),
        R(fn, b, {s: 1}, {s: 0}, f"{fn}: bad extents"),
        R(fn, b, {s: I31 if fn != QUAD else 32768}, {s: 1 << 31}, f"{fn}: bad extents"),  # (QUAD: C*C < 2^31 has a row below)
        R(fn, b, {"B": 0}, {"B": -1}, f"{fn}: bad extents"),
        R(fn, b, {"T": 1}, {"T": 0}, f"{fn}: bad extents"),
        R(fn, b, {"D": 1}, {"D": 0}, f"{fn}: bad extents"),
        R(fn, b, {"V": 1}, {"V": 0}, f"{fn}: bad extents"),
        # B*T < 2^31 and V*D < 2^31 (the kernels index positions and table elements in 32 bits)
        R(fn, b, {"B": I31, "T": 1}, {"B": 1 << 31, "T": 1}, f"{fn}: extent too large"),
        R(fn, b, {"B": 1 << 15, "T": (1 << 16) - 1}, {"B": 1 << 15, "T": 1 << 16}, f"{fn}: extent too large"),
        R(fn, b, {"V": (1 << 29) - 1, "D": 4, **wide}, {"V": 1 << 29, "D": 4, **wide}, f"{fn}: extent too large"),
        # (the diagonal kernel's grid.y ends far below: its last accepted D has a row of its own)
        R(fn, b, None if fn == DIAG else {"V": 1, "D": I31, **wide}, {"V": 1, "D": 1 << 31, **wide}, f"{fn}: extent too large"),
    ]


ROWS = _shared(JAC) + _shared(DIAG) + _shared(QUAD) + [
    # the columns of the weight inside Js
    R(JAC, BASE[JAC], {"col0": 0}, {"col0": -1}, "lk_jac_embed_f32: column range outside Js"),
    R(JAC, BASE[JAC], {"P": 22}, {"P": 21}, "lk_jac_embed_f32: column range outside Js"),
    R(JAC, BASE[JAC], {"col0": 4}, {"col0": 5}, "lk_jac_embed_f32: column range outside Js"),
    # grid.y of the diagonal kernel: 16 lanes x 65535 chunks of d (4-byte accesses when D is no multiple of 4)
    R(DIAG, BASE[DIAG], {"V": 1, "D": 65535 * 16 - 1}, {"V": 1, "D": 65535 * 16 + 1}, "lk_diag_embed_f32: D too large for grid.y"),
    R(QUAD, BASE[QUAD], None, {"var": None}, "lk_diag_quadform_embed_f32: null pointer (var)"),
    R(QUAD, BASE[QUAD], {"C": 32768}, {"C": 32769}, "lk_diag_quadform_embed_f32: too many classes"),
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
    variants = {}
    for key, a in {"ok": (2, 3, 7, 4, 1), "S0": (0, 3, 7, 4, 1), "BT": (2, 1 << 16, 1 << 15, 4, 1), "D0": (2, 3, 7, 0, 1)}.items():
        variants[key] = int(P.lib.lk_embed_variant(*a))
    emit({"variants": variants})
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
        elif "variants" in obj:
            rows["variants"] = obj["variants"]
        elif "done" in obj:
            done = True
    if proc.returncode != 0 or not done:
        pytest.fail(f"the probing child ended with status {proc.returncode}; last probe started: {last}\n" + proc.stderr[-2000:])
    return rows


def _row_id(i):
    return (ROWS[i]["fn"][3:-4] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items()))[:100]


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")


@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_guard_edges(probes, i):
    """first refused -> LK_EINVAL with the guard's own message; last accepted -> anything but a refusal (no device: a call that
    passes the checker ends in LK_ELAUNCH - no launch was made -, or LK_OK for an empty batch)"""
    row = ROWS[i]
    rc, msg = probes[(i, "refuse")]
    assert rc == LK_EINVAL, f"accepted {row['refuse']} (rc={rc}: {msg})"
    assert row["fragment"] in msg, f"refused {row['refuse']} with another message: {msg}"
    if row["accept"] is not None:
        rc, msg = probes[(i, "accept")]
        assert rc in (LK_OK, LK_ELAUNCH), f"refused the in-contract {row['accept']}: rc={rc} {msg}"
        assert row["fn"] not in msg or "kernel" in msg, msg  # (only a failed launch may name this entry point's kernels)
        if row["accept"].get("B") == 0:
            assert rc == LK_OK  # (B == 0 returns before any launch)


def test_variant_refuses_what_the_entry_points_refuse(probes):
    v = probes["variants"]
    assert v["ok"] >= 0 and v["S0"] < 0 and v["BT"] < 0 and v["D0"] < 0


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_embed.hip")).read()
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
    """every LK_REQUIRE of lk_embed.hip: some row's first-refused call came back with that guard's message - the guards of the
    shared checker (``%s: ...``) through each of the three entry points"""
    messages = _guard_messages()
    assert len(messages) >= 7, messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    literal = lambda msg: msg.split(" (")[0]  # noqa: E731  (the text before the parenthesised hint)
    missing = []
    for msg in messages:
        wants = [msg.replace("%s", fn) for fn in FNS] if msg.startswith("%s: ") else [msg]
        assert all(w.startswith(FNS) for w in wants), msg
        missing += [w for w in wants if not any(got.startswith(literal(w)) for got in refused)]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_points_check_through_the_checkers_only():
    """the shape the other file's parser relies on: no guard in an extern "C" body, the checker called before any launch"""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_embed.hip")).read())
    first = text.index('extern "C"')
    assert "LK_REQUIRE" not in text[first:] and "LK_EINVAL" not in text[first:]
    for fn, checker in ((JAC, "jac_embed_check("), (DIAG, "diag_embed_check("), (QUAD, "quad_embed_check(")):
        body = text[text.index(f'extern "C" int {fn}'):]
        assert body.index(checker) < body.index("hipLaunchKernelGGL")


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
