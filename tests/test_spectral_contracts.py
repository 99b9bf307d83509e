"""The argument contracts of the four lk_spectral_* entry points (csrc/lk_spectral.hip), probed at their edges WITHOUT a device -
the method of tests/test_capi_contracts.py (whose helpers are reused) and tests/test_capi_contracts_gate.py: a table of
last-accepted / first-refused values and a child process that sees no device.  Every check lives in ``spectral_check_args``, which
the entry points call before the first HIP call; without a device a call that passes ends in LK_ELAUNCH, or in LK_OK when there
are no samples."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_capi_contracts import LK_EINVAL, LK_ELAUNCH, LK_OK, R, header_prototypes, _Probe  # noqa: E402

QLL, GLL, QR, GR = "lk_spectral_quadform_ll_f32", "lk_spectral_grid_ll_f32", "lk_spectral_quadform_f32", "lk_spectral_grid_f32"
# buffers far from each other: no probe of an extent meets the overlap guard
PHI, QQ, LAM, DEL, OUT, WS = ((1 << 62) + (i << 56) for i in range(6))
BIGWS = 1 << 40
BASE = {
    QLL: dict(phi=PHI, Q=QQ, lam=LAM, hfac=1.0, delta=DEL, B=4, C=3, D=8, has_bias=1, fvar=OUT, ws=WS, ws_bytes=BIGWS),
    GLL: dict(phi=PHI, Q=QQ, lam=LAM, hfac=1.0, deltas=DEL, G=5, B=4, C=3, D=8, has_bias=1, var=OUT, ws=WS, ws_bytes=BIGWS),
    QR: dict(R=PHI, lam=LAM, hfac=1.0, delta=DEL, N=4, C=3, P=8, fvar=OUT, ws=WS, ws_bytes=BIGWS),
    GR: dict(R=PHI, lam=LAM, hfac=1.0, deltas=DEL, G=5, N=4, C=3, P=8, var=OUT, ws=WS, ws_bytes=BIGWS),
}
NAMES = {QLL: ("phi", "B", "delta", "fvar"), GLL: ("phi", "B", "deltas", "var"), QR: ("R", "N", "delta", "fvar"), GR: ("R", "N", "deltas", "var")}


def _rows(fn):
    b = BASE[fn]
    x, n, d, out = NAMES[fn]
    ll, grid = fn in (QLL, GLL), fn in (GLL, GR)
    rows = [R(fn, b, None, {name: None}, f"{fn}: null pointer (") for name in ((x, "lam", d, out) + (("Q",) if ll else ()))]
    ext = f"{fn}: extent out of range (0 <= {n}"
    rows += [
        R(fn, b, {n: 0}, {n: -1}, ext),  # no samples: LK_OK before any HIP call
        R(fn, b, {n: (1 << 24) - 1}, {n: 1 << 24}, ext),
        R(fn, b, {"C": 1}, {"C": 0}, ext),
        R(fn, {**b, **({"D": 1, "has_bias": 0} if ll else {})}, {"C": (1 << 15) - 1}, {"C": 1 << 15}, ext),
        R(fn, b, {"hfac": 1e-30}, {"hfac": 0.0}, f"{fn}: hfac must be positive and finite"),
        R(fn, b, {"hfac": 3.0e38}, {"hfac": float("inf")}, f"{fn}: hfac must be positive and finite"),
        R(fn, b, None, {"hfac": float("nan")}, f"{fn}: hfac must be positive and finite"),
    ]
    if grid:
        rows += [R(fn, b, {"G": 1}, {"G": 0}, ext), R(fn, b, {"G": (1 << 20) - 1}, {"G": 1 << 20}, ext)]
    if ll:
        rows += [
            R(fn, b, {"D": 1}, {"D": 0}, f"{fn}: D out of range (1 <= D <= 896"),
            R(fn, b, {"D": 896, "C": 1}, {"D": 897, "C": 1}, f"{fn}: D out of range (1 <= D <= 896"),
            # P = C D + C <= 32768: 64 (511 + 1) fits, 64 (512 + 1) does not; without the bias row 64 * 512 fits
            R(fn, b, {"C": 64, "D": 511}, {"C": 64, "D": 512}, f"{fn}: P = C D (+ C) out of range"),
            R(fn, {**b, "has_bias": 0}, {"C": 64, "D": 512}, {"C": 65, "D": 512}, f"{fn}: P = C D (+ C) out of range"),
        ]
    else:
        rows += [R(fn, b, {"P": 1}, {"P": 0}, f"{fn}: P out of range (1 <= P <= 32768"),
                 R(fn, b, {"P": 32768, n: 1}, {"P": 32769, n: 1}, f"{fn}: P out of range (1 <= P <= 32768")]
    # the output against its inputs: X at the buffer, the output 4096 bytes on (phi: B 8 floats; R: N 3 8 floats)
    fits = 128 if ll else 42
    rows += [R(fn, {**b, x: "same", out: "other"}, {n: fits}, {n: fits + 1}, f"{fn}: the output overlaps an input or the workspace"),
             R(fn, {**b, "lam": "same"}, {out: "other"}, {out: "same"}, f"{fn}: the output overlaps an input or the workspace"),
             R(fn, {**b, "ws": "same", "ws_bytes": 4096}, {out: "other"}, {out: "same"}, f"{fn}: the output overlaps an input or the workspace")]
    return rows


ROWS = [r for fn in (QLL, GLL, QR, GR) for r in _rows(fn)]
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
    # the workspace guard: one byte short of the advertised size, and the advertised size
    for fn, form in ((QLL, 4), (GLL, 5), (QR, 2), (GR, 3)):
        b = BASE[fn]
        n = b.get("B", b.get("N"))
        need = P.lib.lk_spectral_workspace_bytes(form, n, b["C"], b.get("D", b.get("P")), b.get("G", 1))
        for tag, nbytes in (("short", need - 1), ("exact", need)):
            P.call(*SENTINEL)
            rc, msg = P.call(fn, {**b, "ws_bytes": nbytes})
            emit({"ws": fn, "tag": tag, "rc": rc, "msg": msg, "need": need})
        P.call(*SENTINEL)
        rc, msg = P.call(fn, {**b, "ws": None})
        emit({"ws": fn, "tag": "null", "rc": rc, "msg": msg, "need": need})
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
    rows, ws, last, done = {}, {}, None, False
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
        elif "ws" in obj:
            ws[(obj["ws"], obj["tag"])] = (obj["rc"], obj["msg"], obj["need"])
        elif "done" in obj:
            done = True
    if proc.returncode != 0 or not done:
        pytest.fail(f"the probing child ended with status {proc.returncode}; last probe started: {last}\n" + proc.stderr[-2000:])
    return rows, ws


def _row_id(i):
    return ROWS[i]["fn"][12:] + ":" + ",".join(f"{k}={v}" for k, v in ROWS[i]["refuse"].items())[:60] + f"#{i}"


def test_table_is_well_formed():
    protos = header_prototypes()
    for row in ROWS:
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (side, sorted(set(row[side]) - names))
        assert row["refuse"] and row["fragment"].startswith(row["fn"] + ": ")
    for fn in BASE:
        assert [p[2] for p in protos[fn]] == list(BASE[fn]) + ["stream"]


@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_guard_edges(probes, i):
    """first refused -> LK_EINVAL with the guard's own message; last accepted -> anything but a refusal"""
    rows, _ = probes
    row = ROWS[i]
    rc, msg = rows[(i, "refuse")]
    assert rc == LK_EINVAL, f"accepted {row['refuse']} (rc={rc}: {msg})"
    assert row["fragment"] in msg, f"refused {row['refuse']} with another message: {msg}"
    if row["accept"] is not None:
        rc, msg = rows[(i, "accept")]
        assert rc in (LK_OK, LK_ELAUNCH), f"refused the in-contract {row['accept']}: rc={rc} {msg}"
        a = {**row["base"], **row["accept"]}
        if a.get("B", a.get("N")) == 0:
            assert rc == LK_OK  # (no samples: the call returns before any HIP call)


def test_the_workspace_guard(probes):
    _, ws = probes
    ewf = -2  # LK_EWORKSPACE (include/laplace_hip.h)
    assert "#define LK_EWORKSPACE (-2)" in open(os.path.join(ROOT, "include", "laplace_hip.h")).read()
    for fn in BASE:
        rc, msg, need = ws[(fn, "short")]
        assert need > 0 and rc == ewf and f"{fn}: workspace too small ({need} bytes needed)" in msg
        assert ws[(fn, "null")][0] == ewf
        assert ws[(fn, "exact")][0] in (LK_OK, LK_ELAUNCH)


def test_the_entry_points_check_through_their_checker_only():
    """the shape tests/test_capi_contracts.py's parser relies on: no guard in an extern "C" body"""
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_spectral.hip")).read()
    for fn in BASE:
        body = text[text.index(f'extern "C" int {fn}'):]
        body = body[:body.index("\n}\n")]
        assert "LK_REQUIRE" not in body and "LK_EINVAL" not in body
        assert body.index("spectral_check_args(") < body.index("spectral_run_")
    from tests.test_capi_contracts import guarded_entry_points

    assert not set(BASE) & guarded_entry_points()


def test_workspace_sizes_are_monotone():
    from laplace_amd._lib import HipKernels

    lib = HipKernels().lib
    for form, dp in ((0, 33), (1, 33), (4, 33), (5, 33), (2, 300), (3, 300)):
        f = lambda N, C, G: lib.lk_spectral_workspace_bytes(form, N, C, dp, G)  # noqa: E731
        assert f(1, 1, 1) > 0
        prev = 0
        for N in (1, 31, 32, 33, 64, 65, 1000, 9600, 100000):
            cur = f(N, 3, 7)
            assert cur >= prev, (form, N)
            prev = cur
        prev = 0
        for C in (1, 2, 3, 5, 6, 10, 11, 21, 64):
            cur = f(33, C, 7)
            assert cur >= prev, (form, C)
            prev = cur
        if form & 1:
            prev = 0
            for G in (1, 2, 63, 64, 65, 127, 128, 129, 1000):
                cur = f(33, 3, G)
                assert cur >= prev, (form, G)
                prev = cur
            assert f(33, 3, 128) == f(33, 3, 1000)  # larger grids go in launches of 128 points
    assert lib.lk_spectral_workspace_bytes(0, 0, 3, 33, 1) == 0 and lib.lk_spectral_workspace_bytes(9, 4, 3, 33, 1) == 0


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
