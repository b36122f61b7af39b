"""Build + ctypes binding of the project's HIP shared objects: one `LibSpec` per library in the table `LIBS`, and ONE implementation of each operation
(staleness check, build-if-stale, header-version reader, load) that takes a key of the table: `build_lib`, `load_lib`, `header_version` (over `_build_if_stale`, `_load`, `_header_version`, which take the spec).  The per-library names
(`load_x16()`, `build_post()`, `X16_LIB_PATH`, ...) are one-line views of the table, kept where a caller wants them.

There is NO CPU fallback: every entry point of `ops` goes through these libraries, and loading raises if a shared object is missing, lacks a symbol of its
header or implements another ABI version than the header declares.

The libraries, all hipcc --offload-arch=gfx950 (sources under csrc/; `LibSpec.src_dir` marks an extension library, whose sources live under csrc_ext/ and
include the headers of csrc/ and of their own directory):
  hip    libdkt_hip.so    the PRODUCT (include/dkt_abi.h): the default kernel of every call, no measurement switch, no variant instantiation; held at 250 kernels;
  x16    libdkt_x16.so    the front-end calls for 16-bit (bf16 / f16) trunk features (include/dkt_abi_x16.h); apart so that the product ABI stays as it is;
  data   libdkt_data.so   the episode image transform of the image-dataset loader (include/dkt_abi_data.h);
  smk    libdkt_smk.so    the task-resident spectral-mixture kernels of the sine-wave experiment (include/dkt_abi_smk.h);
  gpc    libdkt_gpc.so    Laplace-approximation GP classification at test time, Newton mode finding and prediction (include/dkt_abi_gpc.h);
  loo    libdkt_loo.so    csrc_ext/: the leave-one-out predictive likelihood and its gradients (include/dkt_abi_loo.h; docs/LOO.md);
  post   libdkt_post.so   csrc_ext/: the joint posterior at test time: covariance, test likelihood, samples (include/dkt_abi_post.h; docs/POSTERIOR.md);
  loofs  libdkt_loofs.so  csrc_ext/: the leave-one-out likelihood of the linear kernels in feature space (include/dkt_abi_loofs.h; docs/LOOFS.md);
  diag   libdkt_diag.so   measurement-only kernels (stream ceilings, co-residency spinners, the round-1 register-sweep kernel): no header, no version;
  twins  libdkt_twins.so  the product's sources with -DDKT_TWINS: every pipeline variant and validation twin the defaults were chosen from, selected by the
                          environment switches of DESIGN.md's appendix.  Same ABI.  Tests and A/B tools only (DKT_TWINS=1 + a variant switch).
All but diag and twins are product code, built under the spill budget.  __graft_entry__.build() brings every library up to date: a failure raises, except for
those `LibSpec.best_effort` marks (post .. twins), where it warns -- they are built on first load as well, and raise there.

An object file's cache key hashes its source, every *.h, *.inc and *.def of csrc/ (and of its own directory), include/dkt_abi.h and the ABI header of its own
library -- what the sources include -- so an edit to one library's header recompiles that library only.

Adding a library: one ABI header under include/, one signature dict, one `LibSpec` entry in `LIBS` (+ the one-line `load_*` / `build_*` names its callers want).
"""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import threading
from typing import NamedTuple, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(_ROOT, "include")
SOURCES = ["dkt_gram.hip", "dkt_gram_ep.hip", "dkt_gram_big.hip", "dkt_gram_small.hip", "dkt_classkernel.hip", "dkt_mll.hip", "dkt_mll_mfma.hip", "dkt_mll_h2.hip", "dkt_mll_reg.hip", "dkt_mll_big.hip", "dkt_mll_tiled.hip", "dkt_mll_band.hip", "dkt_objective.hip", "dkt_predict.hip",
           "dkt_spectral.hip", "dkt_frontend.hip", "dkt_frontend_big.hip", "dkt_lowrank.hip", "dkt_mll_rownoise.hip", "dkt_laplace_grad.hip"]
OBJ_DIR = os.path.join(_HERE, "build")

_c_p = ctypes.c_void_p
_c_i = ctypes.c_int
_c_f = ctypes.c_float

# name -> (restype, argtypes); must list EVERY function of include/dkt_abi.h (tests check this).
SIGNATURES = {
    "dkt_abi_version": (_c_i, []),
    "dkt_device_cu_count": (_c_i, []),
    "dkt_reload_env": (None, []),
    "dkt_env_value": (ctypes.c_char_p, [ctypes.c_char_p]),
    "dkt_gram_f32": (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p]),
    "dkt_mll_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i]),
    "dkt_mll_workspace_bytes_for": (ctypes.c_size_t, [_c_i, _c_i, _c_i, ctypes.c_uint]),
    "dkt_mll_f32": (_c_i, [_c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_f, _c_i,
                           ctypes.c_uint, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                           _c_p, ctypes.c_size_t, _c_p]),
    "dkt_objective_f32": (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_p]),
    "dkt_hyper_grads_f32": (_c_i, [_c_p] * 8 + [_c_i, _c_i, _c_p]),
    "dkt_bn_param_grads_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i]),
    "dkt_bn_param_grads_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_p, ctypes.c_size_t, _c_p]),
    "dkt_gram_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p, ctypes.c_uint, _c_p]),
    "dkt_rbf_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_p]),
    "dkt_sqdist_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_p]),
    "dkt_predict_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_predict_per_class_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_predict_var_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_bn_stats_f32": (_c_i, [_c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_f32": (_c_i, [_c_p, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_train_f32": (_c_i, [_c_p, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                   _c_i, _c_i, _c_i, _c_p]),
    "dkt_affine_normalize_f32": (_c_i, [_c_p, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_normalize_bn_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_class_kernel_f32": (_c_i, [_c_p, _c_i, _c_p, _c_i, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_class_kernel_bwd_nsplit": (_c_i, [_c_i, _c_i]),
    "dkt_class_kernel_bwd_f32": (_c_i, [_c_p, _c_p, _c_i, _c_p, _c_i, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_lowrank_supported": (_c_i, [_c_i, _c_i, _c_i]),
    "dkt_lowrank_gram_f32": (_c_i, [_c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_lowrank_noise_floor_f32": (_c_i, [_c_p, _c_p, _c_p, _c_f, _c_i, _c_p, _c_p, _c_i, _c_p]),
    "dkt_lowrank_finish_f32": (_c_i, [_c_p, _c_p, ctypes.c_long] + [_c_p] * 17 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_lowrank_bwd_f32": (_c_i, [_c_p] * 6 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_smk_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_smk_bwd_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_laplace_grad_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i]),
    "dkt_laplace_grad_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long, _c_p, _c_p, ctypes.c_long] + [_c_p] * 5 + [_c_i, _c_i, _c_i, _c_p, ctypes.c_size_t, _c_p]),
    "dkt_mll_rownoise_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i]),
    "dkt_mll_rownoise_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long, _c_p, ctypes.c_long, _c_p, ctypes.c_long] + [_c_p] * 10 + [_c_i, _c_i, _c_i, ctypes.c_uint,
                                    _c_p, ctypes.c_size_t, _c_p]),
    "dkt_dirichlet_proba_f32": (_c_i, [_c_p] * 5 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_rownoise_lowrank_state_bytes": (ctypes.c_size_t, [_c_i, _c_i]),
    "dkt_rownoise_lowrank_f32": (_c_i, [_c_p, _c_p, ctypes.c_long, _c_p, ctypes.c_long] + [_c_p] * 9 + [ctypes.c_size_t, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_rownoise_lowrank_bwd_f32": (_c_i, [_c_p, _c_p, ctypes.c_long, _c_p, ctypes.c_long] + [_c_p] * 4 + [ctypes.c_size_t, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_rownoise_lowrank_predict_f32": (_c_i, [_c_p, _c_p, ctypes.c_size_t] + [_c_p] * 5 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
}
LAPLACE_MAX_N, LAPLACE_MAX_C = 127, 32      # DKT_LAPLACE_MAX_N / _C of include/dkt_abi.h (DKT_ERR_SHAPE outside them): the limits of dkt_gpc_mode_f32,
                                            # and of dkt_mll_rownoise_f32 / dkt_dirichlet_proba_f32

# libdkt_x16.so (include/dkt_abi_x16.h; tests check that this lists every function of the header): each front-end call of SIGNATURES with `int xdtype` after X
X_BF16 = 1
X_F16 = 2
X16_SIGNATURES = {
    "dkt_x16_abi_version": (_c_i, []),
    "dkt_x16_reload_env": (None, []),
    "dkt_x16_env_value": (ctypes.c_char_p, [ctypes.c_char_p]),
    "dkt_bn_stats_x16": (_c_i, [_c_p, _c_i, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_x16": (_c_i, [_c_p, _c_i, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_train_x16": (_c_i, [_c_p, _c_i, _c_p, _c_p, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gram_bn_bwd_x16": (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                   _c_i, _c_i, _c_i, _c_p]),
    "dkt_affine_normalize_x16": (_c_i, [_c_p, _c_i, _c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    "dkt_normalize_bn_bwd_x16": (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
}

# libdkt_data.so (include/dkt_abi_data.h; tests check that this lists every function of the header)
DATA_SIGNATURES = {
    "dkt_data_abi_version": (_c_i, []),
    "dkt_augment_plan": (_c_i, [_c_p, _c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    "dkt_augment_u8": (_c_i, [_c_p, ctypes.c_size_t, _c_p, _c_p, _c_i, _c_p, _c_p, _c_i, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
}
AUG_COLS = 12

# libdkt_smk.so (include/dkt_abi_smk.h; tests check that this lists every function of the header)
SMK_SIGNATURES = {
    "dkt_smk_abi_version": (_c_i, []),
    "dkt_smk_task_f32": (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_smk_task_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i, _c_i]),
    "dkt_smk_task_bwd_f32": (_c_i, [_c_p] * 10 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
}
SMK_MAX_N, SMK_MAX_M, SMK_MAX_D, SMK_MAX_Q = 32, 256, 64, 8      # the limits of include/dkt_abi_smk.h (DKT_ERR_SHAPE outside them)

# libdkt_gpc.so (include/dkt_abi_gpc.h; tests check that this lists every function of the header)
GPC_SIGNATURES = {
    "dkt_gpc_abi_version": (_c_i, []),
    "dkt_gpc_mode_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long, _c_p, ctypes.c_long] + [_c_p] * 6 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
    "dkt_gpc_predict_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long, _c_p, ctypes.c_long, ctypes.c_long] + [_c_p] * 7 + [_c_i, _c_i, _c_i, _c_i, _c_p]),
}
GPC_MAX_N, GPC_MAX_C = 127, 32      # the limits of include/dkt_abi_gpc.h (DKT_ERR_SHAPE outside them)

# libdkt_diag.so has no header: the entries below are bound at load, and callers of its other exports (tools, tests) set their own argtypes on the handle
DIAG_SIGNATURES = {
    "dkt_diag_mll_reg_f32": (_c_i, [_c_p, _c_p, ctypes.c_long, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_f, _c_i, ctypes.c_uint] + [_c_p] * 11),
}

# libdkt_loo.so (include/dkt_abi_loo.h; tests check that this lists every function of the header)
LOO_SIGNATURES = {
    "dkt_loo_abi_version": (_c_i, []),
    "dkt_loo_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long, _c_p, ctypes.c_long] + [_c_p] * 4 + [_c_i, _c_i, _c_i, _c_f, _c_i, ctypes.c_uint] + [_c_p] * 11),
}
LOO_MAX_N, LOO_MAX_C = 127, 32      # the limits of include/dkt_abi_loo.h (DKT_ERR_SHAPE outside them)

# libdkt_post.so (include/dkt_abi_post.h; tests check that this lists every function of the header)
POST_SIGNATURES = {
    "dkt_post_abi_version": (_c_i, []),
    "dkt_posterior_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i, _c_i]),
    "dkt_posterior_f32": (_c_i, [_c_p, ctypes.c_long, ctypes.c_long] * 3 + [_c_p, ctypes.c_long] + [_c_p] * 5 + [_c_i] * 6 + [_c_f, _c_i] + [_c_p] * 11 +
                          [ctypes.c_size_t, _c_p]),
}
POST_MAX_N, POST_MAX_M, POST_MAX_C = 127, 127, 32      # the limits of include/dkt_abi_post.h (DKT_ERR_SHAPE outside them)

# libdkt_loofs.so (include/dkt_abi_loofs.h; tests check that this lists every function of the header)
LOOFS_SIGNATURES = {
    "dkt_loofs_abi_version": (_c_i, []),
    "dkt_loofs_workspace_bytes": (ctypes.c_size_t, [_c_i, _c_i, _c_i, _c_i]),
    "dkt_loofs_f32": (_c_i, [_c_p, _c_p, ctypes.c_long] + [_c_p] * 4 + [_c_i, _c_i, _c_i, _c_i, _c_f, _c_i, ctypes.c_uint] + [_c_p] * 11 + [ctypes.c_size_t, _c_p]),
}
LOOFS_MAX_D, LOOFS_MAX_C, LOOFS_ROWS = 64, 32, 64      # DKT_LOOFS_MAX_D / _C / _ROWS of include/dkt_abi_loofs.h (DKT_ERR_SHAPE outside the first two; any N >= 1)


class LibSpec(NamedTuple):
    """What differs between the libraries; everything below takes one of these."""
    path: str                               # the shared object
    sources: list                           # names under csrc/
    signatures: dict                        # name -> (restype, argtypes), bound at load
    no_fallback: str                        # the last sentence of its not-built error
    header: Optional[str] = None            # its ABI header under include/: hashed into its objects; `signatures` lists every function of it (tests check this)
    version_macro: Optional[str] = None     # ... as the header defines it
    version_symbol: Optional[str] = None    # ... as the library reports it
    reload_symbol: Optional[str] = None     # makes the library re-read its environment switches (ops._sync_env)
    twins: bool = False                     # compiled with -DDKT_TWINS
    spill_budget: bool = True               # SPILL_BUDGET fails the build: product code (not the twins' non-default instantiations, not measurement kernels)
    src_dir: Optional[str] = None           # where `sources` live when not under csrc/ (an extension library)
    best_effort: bool = False               # a failed build of it only warns in __graft_entry__.build() (it is built, and raises, on first load)


def _so(stem: str) -> str:
    return os.path.join(_HERE, "libdkt_%s.so" % stem)


_ABI = dict(header="dkt_abi.h", version_macro="DKT_ABI_VERSION", version_symbol="dkt_abi_version", reload_symbol="dkt_reload_env",
            signatures=SIGNATURES, no_fallback="the DKT hot path has no CPU fallback.")
CSRC_EXT = os.path.join(_HERE, "csrc_ext")
LIBS = {
    "hip": LibSpec(_so("hip"), SOURCES, **_ABI),
    "x16": LibSpec(_so("x16"), ["dkt_frontend_x16.hip"], X16_SIGNATURES, "16-bit trunk features have no fallback.", "dkt_abi_x16.h", "DKT_X16_ABI_VERSION",
                   "dkt_x16_abi_version", "dkt_x16_reload_env"),
    "data": LibSpec(_so("data"), ["dkt_augment.hip"], DATA_SIGNATURES, "image datasets have no CPU fallback.", "dkt_abi_data.h", "DKT_DATA_ABI_VERSION",
                    "dkt_data_abi_version"),
    "smk": LibSpec(_so("smk"), ["dkt_smk_task.hip"], SMK_SIGNATURES, "there is no CPU fallback.", "dkt_abi_smk.h", "DKT_SMK_ABI_VERSION", "dkt_smk_abi_version"),
    "gpc": LibSpec(_so("gpc"), ["dkt_gpc.hip"], GPC_SIGNATURES, "Laplace GP classification on the device has no fallback.", "dkt_abi_gpc.h", "DKT_GPC_ABI_VERSION",
                   "dkt_gpc_abi_version"),
    "loo": LibSpec(_so("loo"), ["dkt_loo.hip"], LOO_SIGNATURES, "the leave-one-out objective has no fallback.", "dkt_abi_loo.h", "DKT_LOO_ABI_VERSION",
                   "dkt_loo_abi_version", src_dir=CSRC_EXT),
    "post": LibSpec(_so("post"), ["dkt_posterior.hip"], POST_SIGNATURES, "the joint posterior has no fallback.", "dkt_abi_post.h", "DKT_POST_ABI_VERSION",
                    "dkt_post_abi_version", src_dir=CSRC_EXT, best_effort=True),
    "loofs": LibSpec(_so("loofs"), ["dkt_loo_lowrank.hip"], LOOFS_SIGNATURES, "the feature-space leave-one-out objective has no fallback.", "dkt_abi_loofs.h",
                     "DKT_LOOFS_ABI_VERSION", "dkt_loofs_abi_version", src_dir=CSRC_EXT, best_effort=True),
    "diag": LibSpec(_so("diag"), ["dkt_diag.hip", "dkt_mll_reg_twin.hip"], DIAG_SIGNATURES, "the measurement kernels have no fallback.", spill_budget=False,
                    best_effort=True),
    "twins": LibSpec(_so("twins"), SOURCES, twins=True, spill_budget=False, best_effort=True, **_ABI),
}
LIB_PATH, TWINS_LIB_PATH, X16_LIB_PATH, DATA_LIB_PATH, SMK_LIB_PATH, GPC_LIB_PATH, LOO_LIB_PATH, POST_LIB_PATH, LOOFS_LIB_PATH = (
    LIBS[k].path for k in ("hip", "twins", "x16", "data", "smk", "gpc", "loo", "post", "loofs"))

BUILT_WITH_PRODUCT = ("x16", "data", "smk", "gpc")          # what build() brings up to date beside "hip"; __graft_entry__.build() does the rest of the table

_lock = threading.Lock()
_libs = {}          # path -> bound CDLL; a library that is not in here yet has not had its staleness check in this process either


def _lib_path() -> str:
    """DKT_AMD_LIB points the loader at an alternative build of the same ABI (A/B measurements of kernel variants)."""
    return os.environ.get("DKT_AMD_LIB") or LIB_PATH


def _flags(twins: bool = False) -> list:
    return (["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
             "-I", INCLUDE, "-I", CSRC] + (["-DDKT_TWINS"] if twins else []) + os.environ.get("DKT_EXTRA_HIPCC_FLAGS", "").split())


# Register-spill budget per kernel of the PRODUCT library (regex on the mangled name -> max VGPR spills); everything else must not spill at all.  The check
# fails the build when a change makes the compiler spill inside a hot loop.  (The twins library carries the non-default instantiations -- NT = 8 MFMA twins
# with up to 188 spilled VGPRs among them -- and is not checked.)
SPILL_BUDGET = {
    # mll_h2e_kernel (wave per episode, the bench kernel since round 3): no entry = 0 spills allowed, at 254 of 256 VGPRs
    r"mll_h2_kernelILi7ELb1ELb1": 20,              # wave per matrix <NT = 7, GRAD, 5 waves per episode> at its 168-VGPR cap (batches < 1024 episodes): 16
    r"mll_h2_kernelILi[67]E": 12,                  # its forward-only / other-class-count instantiations: 8
    # (gram_sym_ep_split_kernel<8, 2, 2, ...>, the unit-row Gram forward for 112 < N <= 128, had 24 here until round 5: the spills sat in the slab loop, every
    #  scratch reload is a vmcnt(0) that drains the prefetch -- built for two workgroups per CU it has none and runs 1.89 -> 1.36 ms per 8192 episodes of 128 x 1600)
    r"gram_sym_ep_split_kernelILi[78]ELi1ELi1": 8,  # the bf16-split default at NT = 7 / 8
    # tile-array factorisation / inverse at 3 workgroups per CU (168 VGPRs), MC = 7 (N >= 384): values parked in scratch around the diagonal-tile sweep, none in the K loop
    r"tiled_factor_kernelILi\dELb1ELi3E": 28,
    r"tiled_invert_kernelILi\dELb1ELb1ELi3E": 24,
    # band reduction (QR + fused pass at 256 VGPRs): lane constants parked at kernel entry; the forward kernel reloads one per QR column, both a few per panel --
    # none inside the tile loop
    r"band_class_kernel": 8,                      # (only a -DDKT_BAND_CLASS_WAVES=6 measurement build spills: 4; the default, 5 waves per SIMD, has none)
    r"band_sym_kernelILb0E": 32,
    r"band_sym_kernelILb1E": 16,
}


def _parse_resource_remarks(text: str) -> dict:
    """-Rpass-analysis=kernel-resource-usage remarks -> {kernel: {vgprs, agprs, sgprs, scratch, vgpr_spill, sgpr_spill, lds, occupancy}}"""
    import re
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def check_resources(usage: dict) -> list:
    """Kernels whose VGPR spill count exceeds their budget (SPILL_BUDGET; default 0)."""
    import re
    bad = []
    floor = int(os.environ.get("DKT_SPILL_BUDGET_FLOOR", "0"))      # experiments with variant builds only (DKT_EXTRA_HIPCC_FLAGS)
    for name, u in usage.items():
        budget = floor
        for pat, b in SPILL_BUDGET.items():
            if re.search(pat, name):
                budget = max(b, floor)
                break
        if u.get("vgpr_spill", 0) > budget:
            bad.append((name, u.get("vgpr_spill", 0), budget))
    return bad


def _read(path: str) -> bytes:
    with open(path, "rb") as fh:
        return fh.read()


def _digest(src: str, spec: LibSpec) -> str:
    """Content hash of a source, the headers it can include (every csrc/*.h, *.inc and *.def, include/dkt_abi.h, its library's own ABI header) and the flags: the
    object cache key (mtimes do not survive a checkout)."""
    import hashlib
    dirs = [CSRC] + ([spec.src_dir] if spec.src_dir else [])          # (an extension library's sources include csrc/'s headers and their own directory's)
    headers = (sorted(os.path.join(d, f) for d in dirs for f in os.listdir(d) if f.endswith((".h", ".inc", ".def"))) +
               [os.path.join(INCLUDE, f) for f in sorted({"dkt_abi.h", spec.header} - {None})])
    h = hashlib.sha256()
    for f in [src] + headers:
        h.update(_read(f))
    h.update(" ".join(_flags(spec.twins)).encode())
    return h.hexdigest()[:20]


def _src(spec: LibSpec, name: str, replace=None) -> str:
    return (replace or {}).get(name, os.path.join(spec.src_dir or CSRC, name))


def _stamp(spec: LibSpec, replace=None) -> str:
    return ";".join(_digest(_src(spec, s, replace), spec) for s in spec.sources)


def _stale(spec: LibSpec) -> bool:
    if not os.path.exists(spec.path) or not os.path.exists(spec.path + ".stamp"):
        return True
    with open(spec.path + ".stamp") as fh:
        return fh.read() != _stamp(spec)


def needs_build() -> bool:
    return not os.environ.get("DKT_AMD_LIB") and _stale(LIBS["hip"])


def _compile_link(spec: LibSpec, target: str = None, replace=None, verbose=False) -> str:
    """One hipcc -c per source (in parallel, objects cached by content hash under build/), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sources, target = spec.sources, target or spec.path
    os.makedirs(OBJ_DIR, exist_ok=True)

    def one(name):
        src = _src(spec, name, replace)
        obj = os.path.join(OBJ_DIR, "%s.%s.o" % (os.path.basename(src), _digest(src, spec)))
        if not os.path.exists(obj) or not os.path.exists(obj + ".res.json"):
            cmd = [hipcc] + _flags(spec.twins) + ["-c", src, "-o", obj + ".tmp"]
            if verbose:
                print(" ".join(cmd))
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError("hipcc failed on %s:\n%s%s" % (name, res.stdout, res.stderr))
            with open(obj + ".res.json", "w") as fh:
                json.dump(_parse_resource_remarks(res.stderr), fh)
            os.replace(obj + ".tmp", obj)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(sources), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(one, sources))
    usage = {}
    for o in objs:
        with open(o + ".res.json") as fh:
            usage.update(json.load(fh))
    with open(os.path.join(OBJ_DIR, os.path.basename(target) + ".resource_usage.json"), "w") as fh:
        json.dump(usage, fh, indent=1, sort_keys=True)
    bad = check_resources(usage) if spec.spill_budget else []
    if bad:
        raise RuntimeError("register spills beyond the budget (deep-kernel-transfer_amd/_lib.py SPILL_BUDGET):\n" +
                           "\n".join("  %s: %d VGPR spills (budget %d)" % b for b in bad))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", target + ".tmp"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(target + ".tmp", target)
    with open(target + ".stamp", "w") as fh:
        fh.write(_stamp(spec, replace))
    if replace is None:
        # superseded objects of the in-tree libraries' sources (a header edit re-hashes every file: the cache would otherwise grow by ~ 20 MB per edit); kept:
        # what each library of LIBS was last linked from (this link's objects + whatever the other libraries' lists name)
        keep_path = os.path.join(OBJ_DIR, os.path.basename(target) + ".objects.json")
        with open(keep_path, "w") as fh:
            json.dump([os.path.basename(o) for o in objs], fh)
        keep = set()
        for f in os.listdir(OBJ_DIR):
            if f.endswith(".objects.json"):
                with open(os.path.join(OBJ_DIR, f)) as fh:
                    keep.update(json.load(fh))
        known = {src for lib in LIBS.values() for src in lib.sources}
        for f in os.listdir(OBJ_DIR):
            base = f[:-len(".res.json")] if f.endswith(".res.json") else f
            if base.endswith(".o") and base not in keep and any(base.startswith(src + ".") for src in known):
                try:
                    os.remove(os.path.join(OBJ_DIR, f))
                except OSError:
                    pass
    return target


def _build_if_stale(spec: LibSpec, verbose: bool = False) -> str:
    return _compile_link(spec, verbose=verbose) if _stale(spec) else spec.path


def build_lib(key: str, verbose: bool = False) -> str:
    """Bring one library of the table up to date; its path."""
    return _build_if_stale(LIBS[key], verbose)


def build(force: bool = False, verbose: bool = False, out: str = None, replace: dict = None) -> str:
    """hipcc --offload-arch=gfx950 -> deep-kernel-transfer_amd/libdkt_hip.so (in-tree), and the other product libraries of csrc/ (x16, data, smk, gpc) brought up
    to date as well (their own stamps: they are built even when the product library is current).  Cross-compiles without a GPU.  `out` / `replace` ({source
    name: other path}) build a variant library for A/B runs (the product library only)."""
    path = LIB_PATH
    if out is not None or force or needs_build():
        if force and os.path.isdir(OBJ_DIR):
            for f in os.listdir(OBJ_DIR):
                if f.endswith(".o"):
                    os.remove(os.path.join(OBJ_DIR, f))
        path = _compile_link(LIBS["hip"], out, replace, verbose)
    if out is None:
        for key in BUILT_WITH_PRODUCT:
            _build_if_stale(LIBS[key], verbose)
    return path


def build_gpc(verbose: bool = False) -> str:
    return build_lib("gpc", verbose)


def build_twins(verbose: bool = False) -> str:
    return build_lib("twins", verbose)


def build_loo(verbose: bool = False) -> str:
    return build_lib("loo", verbose)


def build_post(verbose: bool = False) -> str:
    return build_lib("post", verbose)


def build_loofs(verbose: bool = False) -> str:
    return build_lib("loofs", verbose)


def _header_version(spec: LibSpec) -> int:
    """The ABI version as the library's header under include/ declares it."""
    import re
    with open(os.path.join(INCLUDE, spec.header)) as fh:
        return int(re.search(r"#define\s+%s\s+(\d+)" % spec.version_macro, fh.read()).group(1))


def header_version(key: str) -> int:
    return _header_version(LIBS[key])


def abi_version_of_header() -> int:
    return header_version("hip")


def x16_abi_version_of_header() -> int:
    return header_version("x16")


def data_abi_version_of_header() -> int:
    return header_version("data")


def smk_abi_version_of_header() -> int:
    return header_version("smk")


def gpc_abi_version_of_header() -> int:
    return header_version("gpc")


def loo_abi_version_of_header() -> int:
    return header_version("loo")


def post_abi_version_of_header() -> int:
    return header_version("post")


def loofs_abi_version_of_header() -> int:
    return header_version("loofs")


def device_code_objects(path: str = None) -> list:
    """The gfx950 code objects (ELF images) inside a built library or object file: the uncompressed clang offload bundles of its .hip_fatbin data."""
    import struct
    blob = open(path or LIB_PATH, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], blob.find(magic)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(magic))[0]
        q = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(magic, pos + len(magic))
    return out


_disasm_cache = {}


def device_disassembly(path: str = None) -> list:
    """llvm-objdump -d of every gfx950 code object of a library: a list of texts (cached per path + mtime; the audits below share it)."""
    import tempfile
    path = path or LIB_PATH
    key = (path, os.path.getmtime(path))
    if key not in _disasm_cache:
        objdump = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
        texts = []
        for img in device_code_objects(path):
            with tempfile.NamedTemporaryFile(suffix=".co") as fh:
                fh.write(img)
                fh.flush()
                res = subprocess.run([objdump, "-d", "--no-show-raw-insn", fh.name], capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError("llvm-objdump failed: " + res.stderr[:500])
            texts.append(res.stdout)
        _disasm_cache.clear()
        _disasm_cache[key] = texts
    return _disasm_cache[key]


# what the two disassembly audits below managed to parse (positive controls for their tests: a toolchain that prints branch operands or `// ADDR:` comments
# differently would otherwise make them pass without checking anything)
AUDIT_STATS = {}


def spill_reloads_in_streaming_loops(path: str = None) -> dict:
    """{kernel: number of scratch reloads} for every kernel that reloads a spilled register INSIDE a loop that also issues global / buffer loads.  Scratch traffic
    shares the in-order memory counter, and a reload's wait is `vmcnt(0)`: such a reload drains whatever the loop prefetched, on every trip (round 5: the unit-row Gram
    forward at 112 < N <= 128 ran 1.89 instead of 1.36 ms per 8192 episodes for 24 spilled registers).  Loops = backward branches of the disassembly."""
    import re
    rx_addr = re.compile(r"//\s*([0-9A-Fa-f]+):")
    rx_br = re.compile(r"^\s*s_c?branch\w*\s+(\d+)")
    out = {}
    AUDIT_STATS["branches"] = AUDIT_STATS["backward_branches"] = AUDIT_STATS["kernels"] = 0
    for text in device_disassembly(path):
        kernel, insns = None, []

        def flush():
            if kernel is None or not insns:
                return
            addrs = [a for a, _ in insns]
            worst = 0
            for a, t in insns:
                m = rx_br.match(t)
                if not m:
                    continue
                AUDIT_STATS["branches"] += 1
                off = int(m.group(1))
                off = off - 65536 if off >= 32768 else off
                tgt = a + 4 + 4 * off
                if tgt >= a:
                    continue
                AUDIT_STATS["backward_branches"] += 1
                body = [tt for aa, tt in insns if tgt <= aa <= a]
                nsc = sum("scratch_load" in tt for tt in body)
                if nsc and any(("buffer_load" in tt) or ("global_load" in tt) for tt in body):
                    worst = max(worst, nsc)
            if worst:
                out[kernel] = worst

        for line in text.splitlines():
            if line.endswith(">:"):
                flush()
                kernel, insns = line.split("<")[-1][:-2], []
                AUDIT_STATS["kernels"] += 1
                continue
            m = rx_addr.search(line)
            if m and kernel is not None:
                insns.append((int(m.group(1), 16), line.split("//")[0]))
        flush()
    return out


def unprotected_wide_buffer_stores(path: str = None) -> list:
    """Disassemble the library's device code (llvm-objdump) and list every 12 / 16-byte BUFFER store with a REGISTER in its soffset field whose data
    registers are written by the next VALU instruction.  hipcc's hazard recogniser skips that form of the store (it inserts the wait state only for a
    literal soffset); on gfx950 the store then sends whatever the VALU wrote (round 5: dX of a software-pipelined fused backward came out as run-to-run
    garbage).  The kernels keep the scalar offset in the VGPR offset instead (bstore4, dkt_mfma_tiles.h); this is the audit that they all do."""
    import re
    rx_store = re.compile(r"^\s*buffer_store_dwordx[34]\s+([va])\[(\d+):(\d+)\],\s*\S+,\s*s\[\d+:\d+\],\s*(s\d+|m0|vcc_lo|vcc_hi)\b")
    rx_dst = re.compile(r"^\s*(v_\w+)\s+(([va])\[(\d+):(\d+)\]|([va])(\d+))\b")
    hits = []
    AUDIT_STATS["wide_stores_any"] = AUDIT_STATS["wide_stores_parsed"] = 0
    rx_any = re.compile(r"^\s*buffer_store_dwordx[34]\s+[va]\[(\d+):(\d+)\]")          # (data in VGPRs or in accumulation registers)
    for text in device_disassembly(path):
        kernel, pending = "?", None
        for line in text.splitlines():
            if line.endswith(">:"):
                kernel, pending = line.split("<")[-1][:-2], None
                continue
            text_ = line.split("//")[0]
            if not text_.strip():
                continue
            if pending is not None:
                m = rx_dst.match(text_)
                if m and not m.group(1).startswith(("v_cmp", "v_mfma", "v_readlane", "v_readfirstlane")):
                    cls = m.group(3) or m.group(6)
                    lo, hi = (int(m.group(4)), int(m.group(5))) if m.group(3) else (int(m.group(7)), int(m.group(7)))
                    if cls == pending[3] and lo <= pending[1] and hi >= pending[0]:
                        hits.append((kernel, pending[2].strip(), text_.strip()))
                pending = None
            m = rx_store.match(text_)
            AUDIT_STATS["wide_stores_any"] += ("buffer_store_dwordx3" in text_) or ("buffer_store_dwordx4" in text_)
            AUDIT_STATS["wide_stores_parsed"] += rx_any.match(text_) is not None          # (the operand syntax the audit's regular expressions expect)
            if m:
                pending = (int(m.group(2)), int(m.group(3)), text_, m.group(1))
    return hits


def _load(spec: LibSpec, path: str = None) -> ctypes.CDLL:
    """dlopen a library and bind every entry of its signature table; raises (never falls back) when it cannot be built or loaded, lacks a symbol, or
    implements another ABI version than its header declares.  Without `path`, the library is first brought up to date where the sources are present: once per
    process (a cached handle returns before that), and inside the lock, so that no thread dlopens a file that another one is replacing.  A `path` is loaded as
    it is."""
    with _lock:
        lib = _libs.get(path or spec.path)
        if lib is not None:
            return lib
        if path is None:
            path = _build_if_stale(spec) if os.path.isdir(CSRC) else spec.path
        if not os.path.exists(path):
            raise RuntimeError("%s is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` -- %s" % (path, spec.no_fallback))
        lib = ctypes.CDLL(path)
        for name, (res, args) in spec.signatures.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise RuntimeError("%s lacks symbol %s declared in %s" % (os.path.basename(path), name, "include/" + spec.header if spec.header else "its signature table")) from e
            fn.restype = res
            fn.argtypes = args
        if spec.header is not None:
            want, got = _header_version(spec), int(getattr(lib, spec.version_symbol)())
            if got != want:
                raise RuntimeError("%s implements %s %d, include/%s declares %d: rebuild (python -c 'import __graft_entry__ as g; g.build()')"
                                   % (path, spec.version_macro, got, spec.header, want))
        _libs[path] = lib
        return lib


def load_lib(key: str, path: str = None) -> ctypes.CDLL:
    return _load(LIBS[key], path)


def load(path: str = None) -> ctypes.CDLL:
    """The product library -- or the build of its ABI that `path` / DKT_AMD_LIB names -- as it is: bringing it up to date is build()'s job (one rank's, in a
    multi-process run)."""
    return load_lib("hip", path or _lib_path())


def load_twins() -> ctypes.CDLL:
    return load_lib("twins")


def load_x16() -> ctypes.CDLL:
    return load_lib("x16")


def load_data() -> ctypes.CDLL:
    return load_lib("data")


def load_smk() -> ctypes.CDLL:
    return load_lib("smk")


def load_gpc() -> ctypes.CDLL:
    return load_lib("gpc")


def load_diag() -> ctypes.CDLL:
    return load_lib("diag")


def load_loo() -> ctypes.CDLL:
    return load_lib("loo")


def load_post() -> ctypes.CDLL:
    return load_lib("post")


def load_loofs() -> ctypes.CDLL:
    return load_lib("loofs")


def reload_env(lib) -> None:
    """Make a handle re-read its environment switches: through the reload symbol of the spec whose library it is (any other handle is a build of the product ABI)."""
    spec = next((s for s in LIBS.values() if s.path == lib._name), LIBS["hip"])
    getattr(lib, spec.reload_symbol)()


STATUS = {0: "DKT_OK", -1: "DKT_ERR_BAD_ARG", -2: "DKT_ERR_TOO_LARGE", -3: "DKT_ERR_WORKSPACE", -4: "DKT_ERR_LAUNCH", -5: "DKT_ERR_SHAPE"}


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, STATUS.get(status, "?"), status))
