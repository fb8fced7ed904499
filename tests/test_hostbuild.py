"""The loader of the host builds (tests/hostbuild.py): staleness from the compiler's dependency file, on a throw-away two-line source with
a header next to it, and the arithmetic mode given to a library at load and to every loaded one after."""
from __future__ import annotations

import ctypes as C
import os

from tests import hostbuild as H


def sources(tmp_path):
    (tmp_path / "real.h").write_text("#ifdef CLOUDSC2_SINGLE\ntypedef float real_t;\n#else\ntypedef double real_t;\n#endif\n")
    (tmp_path / "unit.hip").write_text('#include "real.h"\nextern "C" int real_bytes(void) { return (int)sizeof(real_t); }\n')
    return str(tmp_path / "unit.hip"), str(tmp_path / "real.h")


def rebuilt(src, out, **kw) -> bool:
    n = len(H.BUILT)
    assert H.build(src, out, **kw) == out
    return len(H.BUILT) > n


def age(path, seconds):
    """the file's mtime relative to now"""
    t = os.stat(path).st_mtime + seconds
    os.utime(path, (t, t))


def test_staleness_comes_from_the_dependency_file(tmp_path):
    src, header = sources(tmp_path)
    out = str(tmp_path / "libunit.so")
    for f in (src, header):
        age(f, -100.0)
    assert rebuilt(src, out, single=False) and os.path.exists(out) and os.path.exists(out + ".d")
    assert C.CDLL(out).real_bytes() == 8
    assert os.path.basename(header) in open(out + ".d").read(), "the header is a dependency the compiler names"
    assert sorted(os.listdir(tmp_path)) == ["libunit.so", "libunit.so.d", "real.h", "unit.hip"], "no temporary file is left"

    before = os.stat(out).st_mtime_ns
    assert not rebuilt(src, out, single=False) and os.stat(out).st_mtime_ns == before

    age(header, +200.0)  # the header alone: a hand list that names the source would miss it
    assert rebuilt(src, out, single=False)
    age(out, +400.0)
    assert not rebuilt(src, out, single=False)

    os.remove(out + ".d")
    assert rebuilt(src, out, single=False) and os.path.exists(out + ".d")

    # a dependency that is gone: the file still names it, the build runs (and succeeds: the source no longer includes it)
    age(out, +400.0)
    open(src, "w").write('extern "C" int real_bytes(void) { return 8; }\n')
    age(src, -100.0)
    os.remove(header)
    assert os.stat(src).st_mtime <= os.stat(out).st_mtime
    assert rebuilt(src, out, single=False)
    assert "real.h" not in open(out + ".d").read()


def test_single_defines_the_precision_macro(tmp_path):
    src, _ = sources(tmp_path)
    assert C.CDLL(H.build(src, str(tmp_path / "libunit_sp.so"), single=True)).real_bytes() == 4
    assert C.CDLL(H.build(src, str(tmp_path / "libunit.so"), single=False)).real_bytes() == 8


def test_the_mode_reaches_a_library_at_load_and_every_loaded_one_after():
    loaded = dict(H._libs)
    try:
        H.host_lib("")
        H.set_precise(0)
        H._libs.pop(("vjp", H.B.SINGLE), None)  # as never loaded: set_precise below cannot reach it, only the load can
        H.set_precise(1)
        assert H.host_lib("vjp").hostcheck_get_precise() == 1
        assert H.host_lib("").hostcheck_get_precise() == 1
        H.set_precise(0)
        switched = [lib for lib in H._libs.values() if hasattr(lib, "hostcheck_set_precise")]
        assert len(switched) >= 2 and all(lib.hostcheck_get_precise() == 0 for lib in switched)
    finally:
        H.set_precise(0)
        for key, lib in loaded.items():  # the handles the other tests hold stay the ones the loader switches
            H._libs[key] = lib
