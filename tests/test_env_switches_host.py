"""The environment switches of the HIP libraries: one table (csrc/dkt_switches.def), read by the libraries (csrc/dkt_env.h) and by ops; one reload reaches all of it.
Host checks only: nothing here launches a kernel."""
import glob
import os
import re
import subprocess

import pytest

import dkt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = dkt_amd._lib.CSRC

# the two tuples of ops.py before they were derived from the table
PARENT_PRODUCT = {"DKT_GRAM_EP_MINB", "DKT_MLL_H2E_MINB", "DKT_MLL_TILED_CHUNK", "DKT_MLL_F32MFMA"}
PARENT_VARIANT = {"DKT_GRAM_EP", "DKT_GRAM_SPLIT", "DKT_GRAM_EP_BK", "DKT_GRAM_EP_BD", "DKT_GRAM_UNIT_VAR", "DKT_GRAM_SPLIT_VAR", "DKT_GRAM_BWD_UNIT_VAR",
                  "DKT_GRAM_BWD_SPLIT_VAR", "DKT_GRAM_BWD_UNIT_MIND", "DKT_GRAM_BWD_SPLIT_MIND", "DKT_MLL_TILED_F16", "DKT_GRAM_DIST_EP", "DKT_MLL_P2_GUARD",
                  "DKT_MLL_TILED_WRES", "DKT_MLL_TILED_INVRES", "DKT_GRAM_BIG_EP", "DKT_MLL_TILED_WGS", "DKT_GRAM_BWD_ROWS8", "DKT_MLL_TILED_WDMA", "DKT_CLASS_BWD_V4",
                  "DKT_MLL_TILED_WNW", "DKT_GRAM_SMALL", "DKT_BIG_NB", "DKT_GRAM_BN_F16", "DKT_LDS_STAGE_OLD", "DKT_GRAM_SMALL_WG", "DKT_CLASS_BWD_N128", "DKT_GRAM_FEWEP",
                  "DKT_GRAM_SMALL_XR", "DKT_GRAM_SMALL_LDS",
                  "DKT_PAD_AFFNORM", "DKT_PAD_BAND_BACK", "DKT_PAD_BAND_CLASS", "DKT_PAD_BAND_FWD", "DKT_PAD_CK_BWD", "DKT_PAD_CK_FWD", "DKT_PAD_FE_FWD",
                  "DKT_PAD_GRAM_BIG_BWD", "DKT_PAD_GRAM_EP", "DKT_PAD_GRAM_EP_BWD", "DKT_PAD_LR_BWD", "DKT_PAD_LR_FIN", "DKT_PAD_LR_GRAM", "DKT_PAD_NBB",
                  "DKT_PAD_ROWDOT"}


def _table():
    """[(name without DKT_, class)] as the X-macro lines of the table say."""
    lines = [l for l in open(os.path.join(CSRC, "dkt_switches.def")).read().splitlines() if l.strip() and not l.startswith("//")]
    rows = [re.fullmatch(r"X\(([A-Z0-9_]+), (PRODUCT|VARIANT)\)", l) for l in lines]
    assert all(rows), [l for l, m in zip(lines, rows) if not m]                 # nothing but X(NAME, CLASS) lines and comments: no defaults, no parsing
    return [m.groups() for m in rows]


def test_the_table_is_what_ops_routes_and_what_the_parent_listed():
    ops, table = dkt_amd.ops, _table()
    assert len(table) == len({n for n, _ in table}) == 49
    assert ops._PRODUCT_SWITCHES == tuple("DKT_" + n for n, c in table if c == "PRODUCT")
    assert ops._VARIANT_SWITCHES == tuple("DKT_" + n for n, c in table if c == "VARIANT")
    assert ops._ENV_SWITCHES == ops._PRODUCT_SWITCHES + ops._VARIANT_SWITCHES
    assert set(ops._PRODUCT_SWITCHES) == PARENT_PRODUCT and set(ops._VARIANT_SWITCHES) == PARENT_VARIANT
    assert len(PARENT_PRODUCT) + len(PARENT_VARIANT) == 49
    # no name list is left in ops.py: the table is the only place a switch is written down
    src = open(os.path.join(os.path.dirname(CSRC), "ops.py")).read()
    assert not [n for n in ops._ENV_SWITCHES if n != "DKT_MLL_F32MFMA" and '"%s"' % n in src]


def test_every_switch_is_in_the_appendix_of_the_measurements():
    text = open(os.path.join(ROOT, "docs", "MEASUREMENTS.md")).read()
    start = text.index("## Appendix — environment switches")
    end = text.index("\n## ", start + 1)
    appendix = set(re.findall(r"DKT_[A-Z0-9_]+", text[start:end]))
    assert not sorted(set(dkt_amd.ops._ENV_SWITCHES) - appendix)


def test_the_environment_is_read_in_one_place():
    """getenv only in dkt_env.h; the per-file caches' reset functions and dkt_variant_env are gone; every switch name in the sources is the table's."""
    files = sorted(glob.glob(os.path.join(CSRC, "*")))
    assert len(files) > 30
    reload_defs = []
    for path in files:
        text = open(path).read()
        name = os.path.basename(path)
        if name != "dkt_env.h":
            assert "getenv" not in text, name
        assert "dkt_variant_env" not in text, name
        reload_defs += [(name, m) for m in re.findall(r"\b(\w*_reload_env)\s*\([^)]*\)\s*(?:\{|;)", text)]
    assert sorted(reload_defs) == [("dkt_frontend_x16.hip", "dkt_x16_reload_env"), ("dkt_gram_ep.hip", "dkt_reload_env")], reload_defs
    assert "getenv" in open(os.path.join(CSRC, "dkt_env.h")).read()


LIBS = {"product": ("hip", "dkt_env_value", True), "twins": ("twins", "dkt_env_value", False), "x16": ("x16", "dkt_x16_env_value", True)}


@pytest.mark.parametrize("which", sorted(LIBS))
def test_one_reload_reaches_every_switch(which, monkeypatch):
    """Every name of the table set to a sentinel of its own, ONE reload, and the library's snapshot holds it -- DKT_BIG_NB (a function-local static until this
    table existed: no reload reached it) like the rest.  A product build answers NULL for the variant switches: it does not read them."""
    ops, L = dkt_amd.ops, dkt_amd._lib
    key, value_fn, product_only = LIBS[which]
    L.build()
    lib = L._load(L.LIBS[key])
    value = getattr(lib, value_fn)
    table = _table()
    for i, (name, _) in enumerate(table):
        monkeypatch.setenv("DKT_" + name, "s%d-%s" % (i, name[:8].lower()))
    try:
        L.reload_env(lib)
        for i, (name, cls) in enumerate(table):
            want = None if (product_only and cls == "VARIANT") else ("s%d-%s" % (i, name[:8].lower())).encode()
            assert value(name.encode()) == want, (which, name)
        assert value(b"DKT_BIG_NB") is None and value(b"NO_SUCH_SWITCH") is None and value(b"") is None and value(None) is None
        assert (value(b"BIG_NB") is None) == product_only
        for name, _ in table:
            monkeypatch.delenv("DKT_" + name)
        assert value(table[0][0].encode()) is not None                        # ... a snapshot: not before the reload
        L.reload_env(lib)
        for name, _ in table:
            assert value(name.encode()) is None, (which, name)
    finally:
        monkeypatch.undo()
        L.reload_env(lib)
        ops._env_seen.pop(id(lib), None)                                      # the next call through ops compares against the environment afresh


@pytest.mark.parametrize("twins", [False, True])
def test_standalone_program_under_the_sanitizers(twins, tmp_path):
    """tests/env_switches_main.cpp (its own main, dkt_env.h only), host compiler, address + undefined-behaviour sanitizers, run directly."""
    exe = str(tmp_path / "env_switches_main")
    cxx = os.environ.get("CXX", "c++")
    # the sanitizer runtimes linked INTO the program (clang's default; gcc links them dynamically unless told otherwise): it runs as it is, whatever else is loaded
    static = [] if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + \
          ["-I", CSRC, os.path.join(ROOT, "tests", "env_switches_main.cpp"), "-o", exe] + (["-DDKT_TWINS"] if twins else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "dkt_env.h OK (49 switches)" in res.stdout, res.stdout + res.stderr
