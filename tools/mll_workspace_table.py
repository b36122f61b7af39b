"""The workspace queries of the marginal likelihood over the dispatch edges, as a table: dkt_mll_workspace_bytes_for / dkt_mll_workspace_bytes of the product and
the twins library -> tests/golden/mll_workspace_table.npz, which tests/test_mll_dispatch.py compares the libraries against, byte for byte.  Host only (no GPU).

The fixture is the record of the dispatch BEFORE a change to it: run this on the parent commit of such a change and commit what it wrote; never on the code under test.

    python tools/mll_workspace_table.py [--out FILE]

Arrays (uint64 bytes; `lib` = product | twins):
  B, C, N, flags, env_flags    the grid
  <lib>_for [flags, B, C, N]   dkt_mll_workspace_bytes_for, DKT_MLL_F32MFMA unset
  <lib>_any [B, C, N]          dkt_mll_workspace_bytes
  <lib>_env [env_flags, B, C, N]         dkt_mll_workspace_bytes_for with DKT_MLL_F32MFMA=1 (dkt_reload_env), as this build answers
  <lib>_env_launch [env_flags, B, C, N]  the same rows as dkt_mll_f32 treats them with the variable set: it adds DKT_MLL_FORCE_F32MFMA to the call's flags unless
                               they hold E_PER_CLASS / FORCE_GENERIC / FORCE_REG / FORCE_BLOCKED, so this is this build's own answer (variable unset) for those flags.
                               Where _env differs from it, the query sized another route than the launch takes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dkt_amd  # noqa: E402

GRAD, CHOL, GENERIC, REG, BLOCKED, F32MFMA, E_PER_CLASS, TILED, BAND, NO_KAPPA = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
B = (1, 191, 192, 1024, 1030, 2048)                                        # band window (192), wave-per-episode threshold (1024), chunk edges (128, 1024)
C = (1, 2, 11, 12, 32, 33, 64, 65)                                         # band: 2 .. 32, default from 12; tile arrays with gradients: <= 64 (product)
N = (1, 31, 32, 127, 128, 190, 191, 432, 433, 447, 448, 460)               # Cholesky output on the MFMA kernel (31), wave kernels (127), LDS (190), band (432), tile arrays (447)
SINGLE = (GRAD, CHOL, GENERIC, BLOCKED, F32MFMA, E_PER_CLASS, TILED, BAND, NO_KAPPA)
FLAGS = (0,) + SINGLE + tuple(f | GRAD for f in SINGLE if f != GRAD) + tuple(E_PER_CLASS | f for f in (GENERIC, BLOCKED, F32MFMA, TILED, BAND))
ENV_FLAGS = (0,) + SINGLE
OUT = os.path.join(ROOT, "tests", "golden", "mll_workspace_table.npz")


def promoted(flags: int) -> int:
    """The flags of a call as dkt_mll_f32 sees them with DKT_MLL_F32MFMA=1."""
    return flags if flags & (E_PER_CLASS | GENERIC | REG | BLOCKED) else flags | F32MFMA


def query_for(lib, flag_list) -> np.ndarray:
    return np.array([[[[lib.dkt_mll_workspace_bytes_for(b, c, n, f) for n in N] for c in C] for b in B] for f in flag_list], dtype=np.uint64)


def tables(lib) -> dict:
    """Every table of one library, in the order the environment allows: the variable unset first, set last, unset again on the way out."""
    os.environ.pop("DKT_MLL_F32MFMA", None)
    dkt_amd._lib.reload_env(lib)
    out = {"for": query_for(lib, FLAGS),
           "any": np.array([[[lib.dkt_mll_workspace_bytes(b, c, n) for n in N] for c in C] for b in B], dtype=np.uint64),
           "env_launch": query_for(lib, [promoted(f) for f in ENV_FLAGS])}
    os.environ["DKT_MLL_F32MFMA"] = "1"
    try:
        dkt_amd._lib.reload_env(lib)
        out["env"] = query_for(lib, ENV_FLAGS)
    finally:
        del os.environ["DKT_MLL_F32MFMA"]
        dkt_amd._lib.reload_env(lib)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    dkt_amd._lib.build()
    arrays = {"B": np.array(B), "C": np.array(C), "N": np.array(N), "flags": np.array(FLAGS), "env_flags": np.array(ENV_FLAGS)}
    for name, lib in (("product", dkt_amd._lib.load()), ("twins", dkt_amd._lib.load_twins())):
        for key, tab in tables(lib).items():
            arrays["%s_%s" % (name, key)] = tab
        diff = arrays[name + "_env"] != arrays[name + "_env_launch"]
        print("%s: %d rows, %d with DKT_MLL_F32MFMA=1 of which %d are sized for another route than the launch takes"
              % (name, arrays[name + "_for"].size + arrays[name + "_any"].size, diff.size, int(diff.sum())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
