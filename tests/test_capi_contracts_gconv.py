"""The argument contract of lk_jac_gconv_f32 (csrc/lk_gconv.hip), probed at its edges WITHOUT a device - the method of
tests/test_capi_contracts.py (whose helpers are reused), with a table, a child process and a completeness check of its own.

lk_gconv.hip keeps every argument check in ONE checker function that the entry point calls before the first HIP call; the
completeness test of tests/test_capi_contracts.py reads rows only from its own table and therefore does not see this entry
point.  These rows can be folded into that table.
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

FN = "lk_jac_gconv_f32"
# depthwise with channel multiplier 2: Cig = 1, Dkg = 9, weight columns 0..72, bias columns 72..80; OW = 4 -> 4 lanes per row
_DW = dict(B=4, Cc=5, Cin=4, H=4, W=4, Do=8, groups=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, P=96, col0=0, bcol0=72)
# two groups (Cig = 2, Dkg = 18): the tile path
_G2 = dict(_DW, groups=2, P=160, bcol0=144)
I31 = (1 << 31) - 1
ROWS = [
    R(FN, _DW, {"groups": 1, "P": 296, "bcol0": 288}, {"groups": 0}, "lk_jac_gconv_f32: bad arguments"),
    R(FN, _DW, {"Cc": 1}, {"Cc": 0}, "lk_jac_gconv_f32: bad arguments"),
    R(FN, _DW, {"B": 0}, {"B": -1}, "lk_jac_gconv_f32: bad arguments"),
    R(FN, _DW, None, {"g": None}, "lk_jac_gconv_f32: bad arguments"),
    R(FN, _DW, None, {"Js": None}, "lk_jac_gconv_f32: bad arguments"),
    # divisibility
    R(FN, _DW, {"groups": 2, "P": 160, "bcol0": 144}, {"groups": 3}, "lk_jac_gconv_f32: groups must divide Cin and Do"),
    R(FN, _DW, {"Do": 4}, {"Do": 6}, "lk_jac_gconv_f32: groups must divide Cin and Do"),
    R(FN, _DW, {"Cin": 8, "groups": 8}, {"Cin": 6, "groups": 4}, "lk_jac_gconv_f32: groups must divide Cin and Do"),
    # geometry: stride 0 would divide by zero on the host; the index arithmetic of both kernels is 32-bit
    R(FN, _DW, {"sh": 1}, {"sh": 0}, "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"dw": 1}, {"dw": 0}, "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"ph": 0, "pw": 0, "kh": 1, "kw": 1, "P": 16, "bcol0": 8}, {"ph": -1}, "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"H": 32767}, {"H": 32768}, "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"kh": 32767, "ph": 32767, "P": 1 << 20, "bcol0": -1}, {"kh": 32768, "ph": 32767, "P": 1 << 20, "bcol0": -1},
      "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"sw": 32767}, {"sw": 32768}, "lk_jac_gconv_f32: bad geometry"),
    R(FN, _DW, {"H": 1, "W": 1}, {"H": 1, "W": 1, "ph": 0, "pw": 0}, "lk_jac_gconv_f32: empty output"),
    R(FN, _DW, {"dh": 2, "ph": 1, "H": 3}, {"dh": 2, "ph": 1, "H": 2}, "lk_jac_gconv_f32: empty output"),
    # extents that travel as int; Cig * kh * kw is formed in int and rounded up to a multiple of 16 for grid.x
    R(FN, _DW, {"B": I31}, {"B": 1 << 31}, "lk_jac_gconv_f32: extent too large"),
    R(FN, _DW, {"Cc": I31}, {"Cc": 1 << 31}, "lk_jac_gconv_f32: extent too large"),
    R(FN, _DW, {"groups": 1, "Cin": 238609292, "P": 1 << 40, "bcol0": -1}, {"groups": 1, "Cin": 238609293, "P": 1 << 40, "bcol0": -1},
      "lk_jac_gconv_f32: extent too large"),
    # columns
    R(FN, _DW, {"P": 80}, {"P": 79}, "lk_jac_gconv_f32: column range outside Js"),
    R(FN, _DW, {"P": 72, "bcol0": -1}, {"P": 71, "bcol0": -1}, "lk_jac_gconv_f32: column range outside Js"),
    R(FN, _DW, {"col0": 0}, {"col0": -1}, "lk_jac_gconv_f32: column range outside Js"),
    R(FN, _DW, {"bcol0": 72}, {"bcol0": 71}, "lk_jac_gconv_f32: weight and bias columns overlap"),
    R(FN, _DW, {"col0": 8, "bcol0": 0}, {"col0": 7, "bcol0": 0}, "lk_jac_gconv_f32: weight and bias columns overlap"),
    # depthwise path: grid.x = ceil(B * Do / (256 / lanes per row)) < 2^31; 4 lanes per row here, 64 rows per workgroup
    R(FN, _DW, {"B": I31, "Cin": 64, "groups": 64, "Do": 64, "P": 1024, "bcol0": -1},
      {"B": I31, "Cin": 68, "groups": 68, "Do": 68, "P": 1024, "bcol0": -1}, "lk_jac_gconv_f32: too many rows for one launch"),
    # ... which has no limit on B * Cc, and holds at most 49 taps in registers: 56 taps take the tile path and its grid.z
    R(FN, _DW, {"B": 13108, "kh": 7, "kw": 7, "ph": 3, "pw": 3, "P": 400, "bcol0": 392},
      {"B": 13108, "kh": 8, "kw": 7, "ph": 4, "pw": 3, "P": 456, "bcol0": 448}, "lk_jac_gconv_f32: B*C too large for grid.z"),
    # tile path: grid.z = B * Cc, grid.y = groups * ceil(Do / groups / 16)
    R(FN, _G2, {"B": 13107}, {"B": 13108}, "lk_jac_gconv_f32: B*C too large for grid.z"),
    R(FN, _G2, {"groups": 65535, "Cin": 131070, "Do": 65535, "P": 1 << 22, "bcol0": -1},
      {"groups": 65536, "Cin": 131072, "Do": 65536, "P": 1 << 22, "bcol0": -1}, "lk_jac_gconv_f32: too many output tiles for grid.y"),
    R(FN, _G2, {"groups": 2, "Do": 32767 * 16 * 2, "P": 1 << 40, "bcol0": -1}, {"groups": 2, "Do": 32767 * 16 * 2 + 2, "P": 1 << 40, "bcol0": -1},
      "lk_jac_gconv_f32: too many output tiles for grid.y"),
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
            rc, msg = P.call(FN, {**row["base"], **row[side]})
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
    return f"{','.join(f'{k}={v}' for k, v in ROWS[i]['refuse'].items())}"[:100]


def test_table_is_well_formed():
    names = {p[2] for p in header_prototypes()[FN]}
    for row in ROWS:
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(FN + ": ")


@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_guard_edges(probes, i):
    """first refused -> LK_EINVAL with the guard's own message; last accepted -> anything but a refusal (no device: a call that
    passes the checker ends in LK_ELAUNCH, or LK_OK for an empty batch)"""
    row = ROWS[i]
    rc, msg = probes[(i, "refuse")]
    assert rc == LK_EINVAL, f"accepted {row['refuse']} (rc={rc}: {msg})"
    assert row["fragment"] in msg, f"refused {row['refuse']} with another message: {msg}"
    if row["accept"] is not None:
        rc, msg = probes[(i, "accept")]
        assert rc in (LK_OK, LK_ELAUNCH), f"refused the in-contract {row['accept']}: rc={rc} {msg}"
        assert FN not in msg or "kernel" in msg, msg  # (only a failed launch may name this entry point's kernels)


def _guard_messages():
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_gconv.hip")).read()
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
    """every LK_REQUIRE of lk_gconv.hip: some row's first-refused call came back with exactly that guard's message"""
    messages = _guard_messages()
    assert len(messages) >= 9 and all(msg.startswith(FN + ": ") for msg in messages), messages
    refused = {probes[(i, "refuse")][1] for i in range(len(ROWS))}
    literal = lambda msg: msg.split("%")[0]  # noqa: E731  (the text before a format directive)
    missing = [msg for msg in messages if not any(got.startswith(literal(msg)) for got in refused)]
    assert not missing, f"guards no row reaches: {missing}"


def test_the_entry_point_checks_through_the_checker_only():
    """the shape the other file's parser relies on: no guard in the extern "C" body, one call of the checker before any launch"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_gconv.hip")).read()
    body = text[text.index('extern "C" int lk_jac_gconv_f32'):]
    assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
    assert body.index("gconv_check_arguments(") < body.index("hipLaunchKernelGGL")
    assert text.count('extern "C"') == 1


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
