"""What the tools/autograd*_timing.py scripts share, written once: the state every one of them measures on, the three timers, the
rotation of forms inside one process and the alternation of fresh processes.  A module, not a script: the tools import it
(``python tools/<name>.py`` puts tools/ first on sys.path) and keep what they measure -- their steps, byte counts and summaries.
The package is imported where it is used: the summarise modes and the alternations need no library."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the package of the tree this file lies in

PEAK = 8e12  # B/s, HBM3E of one MI355X


def row(ms, bytes_per_column, ngptot):
    return {"ms": round(ms, 4), "bytes_per_column": bytes_per_column,
            "frac_of_8TBps": round(bytes_per_column * ngptot / (ms * 1e-3) / PEAK, 3)}


def setup(ngptot, nproma=128, nlev=137, prepare=True, fp64=True, **param_flags):
    """The synthetic atmosphere resident on the device, QSAT filled, the op's inputs as views of it.  ``prepare``: the library's
    one-time device preparation happens here, not inside the first timed call; ``fp64=False``: either precision is measured."""
    import dwarf_p_cloudsc2_tl_ad_amd as c2
    from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    assert not (fp64 and B.SINGLE), "fp64 measurement"
    tab = c2.synthetic_table(nlev)
    prm = c2.default_params(c2.ceta_from_table(tab), lregcl=True, **param_flags)
    ds = c2.DeviceState.from_table(tab, nproma, ngptot)
    ds.satur(prm)
    x = ds.op_inputs()
    lay = ag.check_layout(x, prm, ngptot)
    if prepare:
        ag._prepare(ds.device)
    return types.SimpleNamespace(tab=tab, prm=prm, ds=ds, x=x, lay=lay, ptsphy=float(ds.ptsphy), dev=ds.device)


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def new(names, lay, dev):
    """empty planes in the library's precision, one per name"""
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    return {n: torch.empty(lay.shape(n), dtype=B.torch_real(), device=dev) for n in names}


def event_ms(step):
    """ms of one call of `step` between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(step, reps, pre=None, warmup=5, ndigits=None):
    """median of `reps` event-timed calls after `warmup` untimed ones; `pre` (untimed) runs before each call"""
    for _ in range(warmup):
        if pre:
            pre()
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if pre:
            pre()
        ms.append(event_ms(step))
    med = statistics.median(ms)
    return med if ndigits is None else round(med, ndigits)


def wall_ms(step):
    """wall-clock ms of one call between two device synchronisations (for steps whose host reads are part of their cost)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    del r
    return (t1 - t0) * 1e3


def rotated(forms, reps, timer, shift):
    """every form once per repetition, repetition r starting at form r % shift -> {name: [ms, ...]}"""
    ms = {k: [] for k in forms}
    names = list(forms)
    for r in range(reps):
        for k in names[r % shift:] + names[:r % shift]:
            ms[k].append(timer(forms[k]))
    return ms


def children(commands, order_pairs=3, timeout=600):
    """Fresh processes in alternation.  ``commands``: name -> (argv, cwd), run in the given order and in the reverse one, ``order_pairs``
    times each, every child under its own time limit.  After a child that did not end well its output tails are printed, nothing
    more is started and its return code is returned; else [{"which", "result"}], ``result`` the child's last stdout line as JSON."""
    runs = []
    for order in (list(commands), list(commands)[::-1]):
        for _ in range(order_pairs):
            for which in order:
                argv, cwd = commands[which]
                r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, cwd=cwd)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    return r.returncode
                runs.append({"which": which, "result": json.loads(r.stdout.strip().splitlines()[-1])})
    return runs


def spread(results, key_path):
    """(max - min) / median over the processes' results of the number at ``key_path`` (a sequence of keys)"""
    vals = []
    for v in results:
        for k in key_path:
            v = v[k]
        vals.append(v)
    return round((max(vals) - min(vals)) / statistics.median(vals), 4)
