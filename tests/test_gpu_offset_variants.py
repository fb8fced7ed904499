"""Both addressing forms of every sweep kernel on the MI355X, and a record of which variant ran.

Every sweep kernel is built with 32-bit byte offsets (C2F_OFF32, chosen by finish() in csrc/cloudsc2_launch.hip when every buffer of the
launch spans less than 4 GiB) and with 64-bit ones (what a large state gets).  tests/offset_variant_checks.py runs every public sweep
launcher once per form (CLOUDSC2_OFF32=0/1, read once per process: two children); here

  * every output plane of the two children has the same bits, NaN tails included -- the two forms have the same floating-point
    dataflow, so bits are the contract (as tests/test_gpu_parity.py::test_offset_variants_give_the_same_bits holds NL / TL / AD to);
  * the launch logs (cloudsc2_debug_launch_log) show that the children really ran the two forms of the same kernels, and
  * a census: every built variant (cloudsc2_variant_built) of the batched, parameter and parameter-Jacobian families, and every
    C2F_SATLIN / C2F_VJP word of the TL and reverse sweeps, was seen launched -- NEVER_LAUNCHED lists what no public launcher produces.

The fp32 library (CLOUDSC2_PRECISION=single in the children) is held to the same at the first shape.

A forced 64-bit run at these sizes never sets the upper 32 bits of an offset.  The second half launches over ONE packed buffer whose
span really reaches 4 GiB (allocated once, never filled whole): loads from its first and last planes, stores to them, the 64-bit word
in the launch log without any environment variable, the bits of the same launch on flat planes, and sentinels in the neighbouring
planes untouched.

Measured on the MI355X (fp64 library): see DESIGN.md, "Tests per component"."""
from __future__ import annotations

import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import offset_variant_checks as ov
from tests.util import ASSIGN, B, OFF32, ROOT, SATLIN, VJP, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

DEV = ov.DEV
NAN = ov.NAN
# Built variants that no public launcher produces, word -> reason, per family; justified from csrc/cloudsc2_launch.hip.  Empty:
#   families 4-8   finish() sets QSAT / PRECISE / EVAP / OFF32 from the call, the batched launchers add 64 x the chunk's directions
#                  (2..cloudsc2_batch_max() each occur for nbatch = 2..max), the parameter launchers add PARLIN and, with satur = 1,
#                  SATLIN (the reverse sweep: ASSIGN | VJP too) -- exactly the words par_variant_valid / batch_kernel_valid /
#                  parjac_variant_valid admit;
#   C2F_SATLIN     tl_launch_impl(satlin) and ad_launch_impl(AdMode.satlin) add it to a word without QSAT, TRAJ, SELFINC -- the eight
#                  words of each table;
#   C2F_VJP        cloudsc2_vjp_launch: ASSIGN | VJP, with QSAT (traj_in->qsat given) or without it (NULL: SATUR evaluated in the
#                  sweep, the qsat adjoint an output of its own), times PRECISE, EVAP, OFF32 -- all sixteen.
NEVER_LAUNCHED: dict = {1: {}, 3: {}, 4: {}, 5: {}, 6: {}, 7: {}, 8: {}}
FAULT_CODES = (124, 134, 137, 139, -6, -9, -11)
_device_trouble = []  # a step of this module that faulted, aborted or ran into its time limit: nothing more is launched after it


def need_a_sound_device():
    if _device_trouble:
        pytest.fail(f"not launched: {_device_trouble[0]}")


def bits(a: np.ndarray) -> np.ndarray:
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---- the two children ----------------------------------------------------------------------------------------------------------------

def run_children(d, env: dict, *args):
    """the two runs of tests/offset_variant_checks.py, one after the other, no retry: [(return code, output, npz or None)] for
    CLOUDSC2_OFF32 = 0, 1; the second is not started if the first did not end well"""
    need_a_sound_device()
    runs = []
    for mode in ("0", "1"):
        f = str(d / f"off32_{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "offset_variant_checks.py"), f, *args],
                               env={**os.environ, **env, "CLOUDSC2_OFF32": mode}, capture_output=True, text=True, timeout=300)
            rc, text = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            rc, text = 124, f"time limit: {e}"
        print(f"{env} CLOUDSC2_OFF32={mode}: return code {rc}\n{text[-2000:]}")
        runs.append((rc, text, np.load(f) if rc == 0 else None))
        if rc != 0:
            if rc in FAULT_CODES:
                _device_trouble.append(f"tests/offset_variant_checks.py with {env} CLOUDSC2_OFF32={mode} ended with {rc}")
            break
    return runs


def clean_up(d, runs):
    for _, _, z in runs:
        if z is not None:
            z.close()
    for f in d.iterdir():  # (some 3 GB per child: not left for pytest's own clean-up, which keeps the last three runs)
        f.unlink()


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """both shapes in the library of this process (fp64 unless CLOUDSC2_PRECISION says otherwise)"""
    d = tmp_path_factory.mktemp("offset_variants")
    runs = run_children(d, {})
    yield runs
    clean_up(d, runs)


@pytest.fixture(scope="module")
def children_fp32(tmp_path_factory):
    """the fp32 library (other launch bounds, the adjoint as two kernels): the first shape, which already launches every variant"""
    d = tmp_path_factory.mktemp("offset_variants_fp32")
    runs = run_children(d, {"CLOUDSC2_PRECISION": "single"}, "small")
    yield runs
    clean_up(d, runs)


def returned_zero(children):
    for mode, (rc, text, _) in zip("01", children):
        assert rc == 0, (f"CLOUDSC2_OFF32={mode}", text[-4000:])
    assert len(children) == 2


def both(children):
    assert len(children) == 2 and all(z is not None for _, _, z in children), "a child did not end well"
    return children[0][2], children[1][2]


def same_bits_in_every_plane(children, nshapes: int):
    z64, z32 = both(children)
    assert set(z64.files) == set(z32.files)
    planes = [k for k in z64.files if not k.startswith("log_") and k != "cases"]
    kmax = B.lib.cloudsc2_batch_max()
    # per case: NL twice; with the derivatives: TL 3 launchers, AD 4, VJP 2, SATUR pair, parameter pairs, batches, Jacobians, Taylor
    launches = {k.split(".")[3] for k in planes}
    want = {"nl_fused", "nl_qsat", "tl_fed", "tl_self", "tl_traj", "ad_accumulate", "ad_assign", "ad_forward", "ad_reverse", "vjp",
            "ad_forward_fused", "vjp_fused_satur", "tl_satur", "vjp_satur", "tl_par0", "tl_par1", "vjp_par0", "vjp_par1", "parjac_qsat",
            "parjac_fused", "taylor"} | {f"{w}_batch{k}" for w in ("tl", "vjp") for k in range(2, kmax + 1)}
    assert launches == want, launches ^ want
    assert list(z64["cases"]) == list(z32["cases"]) and len(z64["cases"]) == nshapes * len(ov.MODES) * len(ov.FLAGSETS)
    differ, nonzero = [], set()
    for k in planes:
        a, b = z64[k], z32[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if not np.array_equal(bits(a), bits(b)):
            differ.append((k, float(np.nanmax(np.abs(a - b))), float(np.nanmax(np.abs(a)))))
        if np.any(np.nan_to_num(a) != 0):
            nonzero.add(k.split(".")[3])
    assert not differ, (len(differ), differ[:20])
    assert nonzero == want, ("launchers whose every plane is zero", want - nonzero)


def logs(children):
    z64, z32 = both(children)
    return [[(int(c), int(f), int(w)) for c, f, w in zip(z["log_case"], z["log_family"], z["log_word"])] for z in (z64, z32)]


def logs_show_the_two_forms(children):
    l64, l32 = logs(children)
    assert len(l64) > 0
    assert all(not w & OFF32 for _, _, w in l64), [e for e in l64 if e[2] & OFF32][:5]
    assert all(w & OFF32 for _, _, w in l32), [e for e in l32 if not e[2] & OFF32][:5]
    assert [(c, f, w & ~OFF32) for c, f, w in l64] == [(c, f, w & ~OFF32) for c, f, w in l32]
    for _, f, w in l64 + l32:
        assert B.lib.cloudsc2_variant_built(f, w) == 1, (f, w)


def census_of_the_launched(children):
    l64, l32 = logs(children)
    seen = {f: set() for f in range(len(B.FAMILIES))}
    for _, f, w in l64 + l32:
        seen[f].add(w)
    built = {f: {w for w in range(1024) if B.lib.cloudsc2_variant_built(f, w) == 1} for f in seen}
    asserted = {f: built[f] for f in (4, 5, 6, 7, 8)}
    asserted[1] = {w for w in built[1] if w & SATLIN}
    asserted[3] = {w for w in built[3] if w & SATLIN or w & VJP}
    assert len(asserted[1]) == 8 and len(asserted[3]) == 8 + 16 and all(w & ASSIGN for w in asserted[3])
    assert all(not NEVER_LAUNCHED[f] for f in (4, 5, 6, 7, 8)), "the list must stay empty for the batched and parameter families"
    for f, words in sorted(asserted.items()):
        excused = set(NEVER_LAUNCHED[f])
        assert excused <= words and not excused & seen[f], (B.FAMILIES[f], "an excused word that is not built, or was launched after all")
        missing = sorted(words - seen[f] - excused)
        assert not missing, (B.FAMILIES[f], "built, launchable and never launched", missing)
    for f in sorted(seen):
        rest = sorted(built[f] - seen[f])
        print(f"{B.FAMILIES[f]:10s} built {len(built[f]):3d}  launched {len(seen[f] & built[f]):3d}  not launched: {rest}")


def test_both_children_return_zero(children):
    returned_zero(children)


def test_every_plane_has_the_same_bits_in_both_forms(children):
    same_bits_in_every_plane(children, len(ov.SHAPES))


def test_the_logs_show_the_two_forms_of_the_same_kernels(children):
    logs_show_the_two_forms(children)


def test_census_of_the_variants_seen_launched(children):
    census_of_the_launched(children)


def test_the_fp32_library_in_both_forms(children_fp32):
    """The fp32 kernels are other code (launch bounds of three waves per SIMD for the 32-bit TL forms, the adjoint as two kernels):
    the same four statements for libcloudsc2_hip_sp.so, whose variant tables are the fp64 library's."""
    returned_zero(children_fp32)
    assert both(children_fp32)[0]["n32x100.m1.plain.nl_fused.tent"].dtype == np.float32
    same_bits_in_every_plane(children_fp32, 1)
    logs_show_the_two_forms(children_fp32)
    census_of_the_launched(children_fp32)


# ---- the launch log on the device ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    need_a_sound_device()
    tab = c2.random_table(137, 100, seed=5)
    prm = c2.default_params(c2.ceta_from_table(tab))
    prm.math_mode = 1  # (the word below: no PRECISE whatever the process default)
    st = c2.state_from_table(tab, 32, 100)
    lay = ag.Layout(st.nblocks, st.nlev, 32, 100)
    x = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
    return x, prm, float(st.ptsphy), lay


def test_the_log_counts_on_when_it_is_full_and_is_the_calling_threads_own(small):
    x, prm, ptsphy, lay = small
    out = ov.packed("out", B.OUT_NAMES, lay)
    word = 0 if "CLOUDSC2_OFF32" in os.environ and int(os.environ["CLOUDSC2_OFF32"]) == 0 else OFF32
    B.launch_log_reset()
    other = []

    def elsewhere():  # launches on another thread are that thread's
        B.launch_log_reset()
        with torch.cuda.device(DEV):
            ov.nl(x, prm, ptsphy, lay, out=ov.packed("out", B.OUT_NAMES, lay))
            torch.cuda.synchronize()
        other.append(B.launch_log())

    t = threading.Thread(target=elsewhere)
    t.start()
    t.join()
    assert other == [[(0, word)]] and B.launch_log() == []
    for j in range(B.LAUNCH_LOG_MAX + 6):
        ov.nl(x, prm, ptsphy, lay, out=out)
        if j == 2:
            assert B.launch_log() == [(0, word)] * 3
    torch.cuda.synchronize()
    import ctypes as C

    fam, wrd = (C.c_int * 80)(*([-7] * 80)), (C.c_uint * 80)(*([77] * 80))
    assert B.lib.cloudsc2_debug_launch_log(fam, wrd, 80) == B.LAUNCH_LOG_MAX + 6  # counted on, the record incomplete
    assert list(fam) == [0] * B.LAUNCH_LOG_MAX + [-7] * 16 and list(wrd) == [word] * B.LAUNCH_LOG_MAX + [77] * 16
    with pytest.raises(c2.Cloudsc2Error):
        B.launch_log()
    assert B.lib.cloudsc2_debug_launch_log(fam, wrd, 2) == B.LAUNCH_LOG_MAX + 6
    B.launch_log_reset()
    assert B.launch_log() == []


def test_a_launch_under_stream_capture_is_logged_once_and_replays_are_not(small):
    x, prm, ptsphy, lay = small
    out = ov.packed("out", B.OUT_NAMES, lay)
    want = ov.nl(x, prm, ptsphy, lay)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    B.launch_log_reset()
    with torch.cuda.graph(g):
        ov.nl(x, prm, ptsphy, lay, out=out)
    captured = B.launch_log()
    assert len(captured) == 1 and captured[0][0] == 0
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert B.launch_log() == captured
    for n in B.OUT_NAMES:
        assert np.array_equal(bits(out[n].cpu().numpy()), bits(want[n].cpu().numpy())), n


# ---- true spans of 4 GiB and more ----------------------------------------------------------------------------------------------------

NPROMA, NGPTOT = 128, 1024
SENTINEL = -12345.5
LAUNCHERS = ("vjp", "tl_satur", "vjp_satur", "tl_par0", "tl_par1", "vjp_par0", "vjp_par1", "parjac")


@pytest.fixture(scope="module")
def big():
    """one (nblocks, planes, nlev, nproma) buffer whose blocks span 4 GiB, never filled whole; freed at module end"""
    need_a_sound_device()
    esize = torch.empty((), dtype=B.torch_real()).element_size()
    nblocks, nlev = NGPTOT // NPROMA, 137
    planes = -(-(1 << 32) // (esize * nblocks * nlev * NPROMA))
    buf = torch.empty((nblocks, planes, nlev, NPROMA), dtype=B.torch_real(), device=DEV)
    assert buf.stride(0) * nblocks * esize >= 1 << 32 and nblocks == 8
    yield buf
    del buf
    torch.cuda.empty_cache()


_setups: dict = {}


def setup(levapls2: bool):
    """the state, a tangent, a cotangent and the trajectory passes at NPROMA 128 x 1024 columns on flat planes, once per flag set"""
    if levapls2 not in _setups:
        tab = c2.random_table(137, 100, seed=5)
        prm = c2.default_params(c2.ceta_from_table(tab), levapls2=levapls2)
        st = c2.state_from_table(tab, NPROMA, NGPTOT)
        lay = ag.Layout(st.nblocks, st.nlev, NPROMA, NGPTOT)
        ptsphy = float(st.ptsphy)
        x = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
        x["qsat"] = ag.satur(x["pap"], x["t"], prm, NGPTOT)
        x = {n: x[n] for n in B.IN_NAMES}
        x15 = {n: x[n] for n in ov.IN15}
        dx = ov.seeded(B.IN_NAMES, lay, 100, scale=x)
        u = ov.seeded(B.OUT_NAMES, lay, 200)
        _setups[levapls2] = dict(prm=prm, lay=lay, ptsphy=ptsphy, x=x, x15=x15, dx=dx, u=u, fwd=ov.ad_forward(x, prm, ptsphy, lay),
                                 fwd15=ov.ad_forward(x15, prm, ptsphy, lay))
        torch.cuda.synchronize()
    return _setups[levapls2]


def flat(names, lay):
    return {n: torch.full(lay.shape(n), NAN, dtype=B.torch_real(), device=DEV) for n in names}


def run_launcher(which: str, s: dict, x: dict, into: dict | None):
    """one launch on the trajectory `x`; `into`: views that replace some of the launch's NaN-prefilled flat output planes.  -> the planes
    the launch writes, by name, and its entries in the launch log"""
    prm, lay, ptsphy, u = s["prm"], s["lay"], s["ptsphy"], s["u"]
    satur = which.endswith("satur") or which.endswith("1")
    names = ov.IN15 if satur else B.IN_NAMES
    xs = {n: x[n] for n in names}
    dxs = {n: s["dx"][n] for n in names}
    traj, sc = s["fwd15"] if satur else s["fwd"]
    dpar = [0.01 * getattr(prm, n) for n in ov.P]
    B.launch_log_reset()
    if which in ("vjp", "vjp_satur"):
        out = ov.vjp(xs, traj, sc, u, prm, ptsphy, lay, satur=satur, xa=dict(flat(names, lay), **(into or {})))
    elif which == "tl_satur":
        out = ov.tl_satur(xs, dxs, prm, ptsphy, lay, dy=dict(flat(B.OUT_NAMES, lay), **(into or {})))
    elif which.startswith("tl_par"):
        out = ov.tl_par(xs, dxs, dpar, prm, ptsphy, lay, int(satur), dy=dict(flat(B.OUT_NAMES, lay), **(into or {})))
    elif which.startswith("vjp_par"):
        out, work, par_adj = ov.vjp_par(xs, traj, sc, u, prm, ptsphy, lay, int(satur), xa=dict(flat(names, lay), **(into or {})))
        out = dict(out, work=work, par_adj=par_adj)
    else:  # parjac: every block's tendencies share one block stride, so with `into` all of them are views of the one buffer
        ndir = len(ov.P) if prm.levapls2 else len(ov.P) - 1
        sens = [dict(flat(B.OUT_NAMES, lay), **(into[k] if into else {})) for k in range(len(ov.P))]
        ov.parjac(xs, prm, ptsphy, lay, sens=sens)
        out = {f"{k}.{n}": t for k in range(ndir) for n, t in sens[k].items()}
    return out, B.launch_log()


@pytest.mark.parametrize("case", ["loads", "stores"])
@pytest.mark.parametrize("levapls2", [False, True])
@pytest.mark.parametrize("which", LAUNCHERS)
def test_spans_of_4_gib(big, which, levapls2, case):
    need_a_sound_device()
    s = setup(levapls2)
    lay = s["lay"]
    last = big.shape[1] - 1
    want, log_flat = run_launcher(which, s, s["x"], None)
    big[:, 1] = SENTINEL
    big[:, last - 1] = SENTINEL
    into, x = None, s["x"]
    if case == "loads":  # the trajectory's l / i in the first and the last plane
        big[:, 0] = s["x"]["l"]
        big[:, last] = s["x"]["i"]
        x = dict(s["x"], l=big[:, 0], i=big[:, last])
    else:                # the group the launch writes in the buffer, its last field in the last plane
        ndir = len(ov.P) if levapls2 else len(ov.P) - 1
        if which == "parjac":
            spots = [{"tent": 4 * k + 4, "tenq": 4 * k + 5, "tenl": 4 * k + 6, "teni": last if k == ndir - 1 else 4 * k + 7} for k in range(len(ov.P))]
            spots[0]["tent"] = 0
            into = [{n: big[:, p] for n, p in sp.items()} for sp in spots]
            used = [t for d in into for t in d.values()]
        elif which.startswith("vjp"):
            into = {"l": big[:, 0], "i": big[:, last]}
            used = list(into.values())
        else:
            into = {"tent": big[:, 0], "tenq": big[:, 2], "tenl": big[:, 3], "teni": big[:, last]}
            used = list(into.values())
        for t in used:
            t.fill_(NAN)
    got, log_big = run_launcher(which, s, x, into)
    torch.cuda.synchronize()
    # the 64-bit form of the kernel the flat launch ran, chosen from the span alone
    assert len(log_big) == len(log_flat) == 1, (log_big, log_flat)
    (fam, word), (fam_flat, word_flat) = log_big[0], log_flat[0]
    assert not word & OFF32, (which, "the launch over a 4 GiB span took the 32-bit offsets", word)
    assert fam == fam_flat == {"vjp": 3, "tl_satur": 1, "vjp_satur": 3, "tl_par0": 7, "tl_par1": 7, "vjp_par0": 8, "vjp_par1": 8, "parjac": 6}[which]
    assert word == word_flat & ~OFF32
    if "CLOUDSC2_OFF32" not in os.environ:
        assert word_flat & OFF32
    assert set(got) == set(want)
    for n in want:
        assert ov_same_bits(got[n], want[n]), (which, "not the bits of the launch on flat planes", n)
    assert any(bool(torch.any(torch.nan_to_num(t) != 0)) for t in want.values())
    for p in (1, last - 1):
        assert bool(torch.all(big[:, p] == SENTINEL)), (which, "a neighbouring plane of the buffer was written", p)


def ov_same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    v = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))
