"""CPU-side checks of the loader table (dkt_amd._lib.LIBS): which sources and headers belong to which library, and what the one load path does for each."""
import os
import re

import pytest

import dkt_amd

L, ops = dkt_amd._lib, dkt_amd.ops


KEYS = ["data", "diag", "gpc", "hip", "loo", "loofs", "post", "smk", "twins", "x16"]
EXTENSIONS = ["loo", "loofs", "post"]


def test_the_table_holds_every_library():
    assert sorted(L.LIBS) == KEYS
    assert sorted(k for k, spec in L.LIBS.items() if spec.src_dir) == EXTENSIONS and all(L.LIBS[k].src_dir == L.CSRC_EXT for k in EXTENSIONS)
    assert len({spec.path for spec in L.LIBS.values()}) == len(KEYS)
    # what a failed build of only warns about in __graft_entry__.build(); product code is built under the spill budget
    assert sorted(k for k, spec in L.LIBS.items() if spec.best_effort) == ["diag", "loofs", "post", "twins"]
    assert sorted(k for k, spec in L.LIBS.items() if not spec.spill_budget) == ["diag", "twins"]
    # what build() brings up to date itself; __graft_entry__.build() loops over the rest
    assert L.BUILT_WITH_PRODUCT == ("x16", "data", "smk", "gpc") and not [k for k in L.BUILT_WITH_PRODUCT if L.LIBS[k].best_effort or L.LIBS[k].src_dir]
    assert [name for name in vars(L) if isinstance(getattr(L, name), L.LibSpec)] == []          # no spec stands beside the table


def test_every_source_belongs_to_exactly_one_library():
    for src_dir in (L.CSRC, L.CSRC_EXT):
        owned = [s for key, spec in L.LIBS.items() if key != "twins" and (spec.src_dir or L.CSRC) == src_dir for s in spec.sources]
        assert sorted(owned) == sorted(f for f in os.listdir(src_dir) if f.endswith(".hip")), src_dir
    assert L.LIBS["twins"].sources is L.LIBS["hip"].sources


def test_every_signature_table_is_its_header():
    """For every library with a header: the functions the header declares are the keys of its signature table, with as many arguments."""
    seen = 0
    for key, spec in L.LIBS.items():
        if spec.header is None:
            continue
        flat = re.sub(r"/\*.*?\*/", "", open(os.path.join(L.INCLUDE, spec.header)).read(), flags=re.S)
        assert sorted(set(re.findall(r"\b(dkt_\w+)\s*\(", flat))) == sorted(spec.signatures), key
        for name, (_, args) in spec.signatures.items():
            proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1).strip()
            assert len(args) == (0 if proto == "void" else proto.count(",") + 1), (key, name)
        assert spec.version_symbol in spec.signatures and L.header_version(key) >= 1, key
        seen += 1
    assert seen == len(KEYS) - 1 and L.LIBS["diag"].header is None


def _stamp_with_edited(monkeypatch, key, header=None):
    """The stamp of a library as it would be after an edit to include/<header>."""
    read, edited = L._read, header and os.path.join(L.INCLUDE, header)
    with monkeypatch.context() as m:
        m.setattr(L, "_read", lambda path: read(path) + (b"// edited\n" if path == edited else b""))
        return L._stamp(L.LIBS[key])


@pytest.mark.parametrize("key, header, changes", [("hip", "dkt_abi.h", True), ("hip", "dkt_abi_x16.h", False),
                                                  ("smk", "dkt_abi_smk.h", True), ("smk", "dkt_abi.h", True), ("smk", "dkt_abi_data.h", False),
                                                  ("loofs", "dkt_abi_loofs.h", True), ("loofs", "dkt_abi_loo.h", False), ("hip", "dkt_abi_loofs.h", False)])
def test_a_header_edit_restamps_the_libraries_that_include_it(monkeypatch, key, header, changes):
    assert os.path.exists(os.path.join(L.INCLUDE, header))
    assert (_stamp_with_edited(monkeypatch, key, header) != _stamp_with_edited(monkeypatch, key)) == changes


def test_built_libraries_load_where_the_sources_are_absent(lib, monkeypatch):
    def no_build(*args, **kwargs):
        raise AssertionError("a build was attempted")

    monkeypatch.setattr(L, "CSRC", os.path.join(L.CSRC, "absent"))
    monkeypatch.setattr(L, "_compile_link", no_build)
    monkeypatch.delitem(L._libs, L.SMK_LIB_PATH, raising=False)          # first load of this process: the staleness check would run
    smk = L.load_smk()
    assert smk.dkt_smk_abi_version() == L.smk_abi_version_of_header()
    assert smk.dkt_smk_task_f32.argtypes == L.SMK_SIGNATURES["dkt_smk_task_f32"][1]


def test_diag_handle_is_cached_and_bound():
    diag = L.load_diag()
    assert L.load_diag() is diag
    assert diag.dkt_diag_mll_reg_f32.argtypes == L.DIAG_SIGNATURES["dkt_diag_mll_reg_f32"][1]


def test_env_sync_calls_the_reload_entry_of_the_handles_library(monkeypatch):
    """ops._sync_env on a handle of libdkt_x16.so calls dkt_x16_reload_env (tests/test_abi_host.py has the product's dkt_reload_env)."""
    class Stub:
        _name = L.X16_LIB_PATH
        reloads = 0

        def dkt_x16_reload_env(self):
            Stub.reloads += 1

    stub = Stub()
    monkeypatch.setattr(ops, "_env_seen", {})
    for k in ops._ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ops._sync_env(stub, ops._PRODUCT_SWITCHES)
    assert Stub.reloads == 0                                       # no switch set when the handle is first seen: nothing to re-read
    monkeypatch.setenv("DKT_MLL_H2E_MINB", "7")
    ops._sync_env(stub, ops._PRODUCT_SWITCHES)
    ops._sync_env(stub, ops._PRODUCT_SWITCHES)
    assert Stub.reloads == 1
