"""The dispatch of dkt_mll_f32 (csrc/dkt_mll.hip, mll_plan): the workspace queries against the table recorded before the planner existed (host only), and the
fall-through of a call whose workspace is too short for its first route (GPU, at the C ABI)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "mll_workspace_table.npz")       # written by tools/mll_workspace_table.py on the commit before the planner


def _table_tool():
    spec = importlib.util.spec_from_file_location("mll_workspace_table", os.path.join(ROOT, "tools", "mll_workspace_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["product", "twins"])
def test_workspace_queries_match_the_recorded_table(lib, name):
    """dkt_mll_workspace_bytes_for / dkt_mll_workspace_bytes over every dispatch edge, byte for byte what the library answered before query and launch shared one
    planner.  With DKT_MLL_F32MFMA=1 the old query did not know that the launch adds DKT_MLL_FORCE_F32MFMA to the flags (so it sized the band reduction where the
    launch took the tile arrays): those rows must equal the recorded answer for the flags the launch really uses (<lib>_env_launch), all others are unchanged."""
    tool, gold = _table_tool(), np.load(TABLE)
    # the grid is part of the contract: the fixture holds exactly these edges
    assert gold["B"].tolist() == [1, 191, 192, 1024, 1030, 2048] and gold["C"].tolist() == [1, 2, 11, 12, 32, 33, 64, 65]
    assert gold["N"].tolist() == [1, 31, 32, 127, 128, 190, 191, 432, 433, 447, 448, 460]
    single = [1, 2, 4, 16, 32, 64, 128, 256, 512]
    assert gold["flags"].tolist() == [0] + single + [f | 1 for f in single[1:]] + [64 | f for f in (4, 16, 32, 128, 256)]
    assert gold["env_flags"].tolist() == [0] + single
    for key in ("B", "C", "N"):
        assert list(getattr(tool, key)) == gold[key].tolist()
    assert list(tool.FLAGS) == gold["flags"].tolist() and list(tool.ENV_FLAGS) == gold["env_flags"].tolist()
    # the known disagreement of the old query, and nothing else: shared-matrix calls in the band reduction's window whose flags the variable promotes
    old_env, launch_env = gold[name + "_env"], gold[name + "_env_launch"]
    fi, bi, ci, ni = np.nonzero(old_env != launch_env)
    assert len(fi) == 192
    assert set(gold["env_flags"][fi].tolist()) <= {0, 1, 256, 512} and set(gold["C"][ci].tolist()) <= {2, 11, 12, 32} and set(gold["N"][ni].tolist()) == {128, 190, 191, 432}
    got = tool.tables(lib if name == "product" else dkt_amd._lib.load_twins())
    for key, want in (("for", "_for"), ("any", "_any"), ("env", "_env_launch"), ("env_launch", "_env_launch")):
        bad = np.argwhere(got[key] != gold[name + want])
        assert len(bad) == 0, (key, len(bad), bad[:8].tolist())


def _unit_row_episodes(cuda, b, c, n, d):
    rng = np.random.default_rng(b * 1000 + n)
    z = rng.standard_normal((b, n, d))
    z = torch.as_tensor(z / np.linalg.norm(z, axis=2, keepdims=True), dtype=torch.float32, device=cuda)
    e = ops.gram(z, None, ops.KERNEL_LINEAR_UNIT)
    y = torch.where(torch.arange(n, device=cuda).unsqueeze(0) % c == torch.arange(c, device=cuda).unsqueeze(1), 1.0, -1.0).contiguous()
    t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32), device=cuda)  # noqa: E731
    return e, y, t(np.linspace(0.7, 1.1, c)), t(np.linspace(-0.1, 0.1, c)), t(np.full(c, 0.1))


def _mll_at_the_abi(lib, ops_in, b, c, n, flags, ws_bytes, null_ws=False):
    """One dkt_mll_f32 call with exactly `ws_bytes` of workspace (or NULL): (status, every output, pre-filled so that an output nobody wrote cannot compare equal)."""
    e, y, sv, mean, noise = ops_in
    dev = e.device
    out = {"logp": (b, c), "alpha": (b, c, n), "w": (b, n, n), "dsv": (b, c), "dmean": (b, c), "dnoise": (b, c), "jit": (b, c)}
    out = {k: torch.full(s, -7.0, device=dev) for k, s in out.items()}
    out["info"] = torch.full((b, c), -7, device=dev, dtype=torch.int32)
    ws = None if null_ws else torch.empty((ws_bytes + 3) // 4 + 1, device=dev, dtype=torch.float32)
    p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    rc = lib.dkt_mll_f32(p(e), p(y), 0, p(sv), p(mean), p(noise), b, c, n, 1e-6, 3, flags, 0, p(out["logp"]), p(out["alpha"]), 0, p(out["w"]), p(out["dsv"]),
                         p(out["dmean"]), p(out["dnoise"]), p(out["jit"]), p(out["info"]), p(ws), 0 if null_ws else ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def _same_bits(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["info"].abs().max().item()) == 0 and not bool((a["logp"] == -7.0).any())


@pytest.mark.gpu
def test_mll_short_band_workspace_falls_through_to_the_tile_arrays(cuda, monkeypatch):
    """DKT_MLL_FORCE_BAND with a workspace one byte short of the band reduction's: DKT_OK, served by the next route of the plan that fits -- the tile arrays --
    bit for bit."""
    monkeypatch.delenv("DKT_MLL_F32MFMA", raising=False)
    lib = ops._lib_now()
    b, c, n, grad = 2, 2, 130, ops.MLL_WANT_GRAD
    band = int(lib.dkt_mll_workspace_bytes_for(b, c, n, grad | ops.MLL_FORCE_BAND))
    tiled = int(lib.dkt_mll_workspace_bytes_for(b, c, n, grad | ops.MLL_FORCE_TILED))
    if not 0 < tiled < band:
        c = 3
        band = int(lib.dkt_mll_workspace_bytes_for(b, c, n, grad | ops.MLL_FORCE_BAND))
        tiled = int(lib.dkt_mll_workspace_bytes_for(b, c, n, grad | ops.MLL_FORCE_TILED))
    assert 0 < tiled < band, (tiled, band)
    x = _unit_row_episodes(cuda, b, c, n, 16)
    rc_t, ref = _mll_at_the_abi(lib, x, b, c, n, grad | ops.MLL_FORCE_TILED, tiled)
    rc_s, short = _mll_at_the_abi(lib, x, b, c, n, grad | ops.MLL_FORCE_BAND, band - 1)
    assert rc_t == 0 and rc_s == 0
    _same_bits(short, ref)


@pytest.mark.gpu
def test_mll_without_a_workspace_takes_the_generic_kernel(cuda, monkeypatch):
    """128 <= N with workspace = NULL: no route that needs scratch fits, the call is the LDS-resident generic kernel's (DKT_MLL_FORCE_GENERIC), bit for bit."""
    monkeypatch.delenv("DKT_MLL_F32MFMA", raising=False)
    lib = ops._lib_now()
    b, c, n, grad = 2, 2, 130, ops.MLL_WANT_GRAD
    assert lib.dkt_mll_workspace_bytes_for(b, c, n, grad | ops.MLL_FORCE_GENERIC) == 0 and lib.dkt_mll_workspace_bytes_for(b, c, n, grad) > 0
    x = _unit_row_episodes(cuda, b, c, n, 16)
    rc_g, ref = _mll_at_the_abi(lib, x, b, c, n, grad | ops.MLL_FORCE_GENERIC, 0, null_ws=True)
    rc_n, none = _mll_at_the_abi(lib, x, b, c, n, grad, 0, null_ws=True)
    assert rc_g == 0 and rc_n == 0
    _same_bits(none, ref)
