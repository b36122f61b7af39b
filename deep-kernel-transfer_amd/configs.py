"""Module-level switches.  The attribute names and values are the reference's (configs.py:1-7) because its callers read them as
`configs.save_dir`, `configs.data_dir[dataset]` and `configs.kernel_type`; nothing else is taken from that file.

kernel_type: 'bncossim' (default), 'cossim', 'linear', 'rbf', 'matern', 'poli1', 'poli2' for classification;
             'rbf' or 'spectral' for regression (the regression drivers fall back to 'rbf' when this names a classification kernel).
"""
kernel_type = 'bncossim'

# mixed-precision backbone of the models a process builds when their constructor is not told (DKT / DKTRegression amp=None): None (fp32) or 'bf16'.
# The drivers' `--amp` flag sets it (io_utils.parse_args), as `--kernel_type` feeds kernel_type.
amp = None

# likelihood of the DKT models a process builds when their constructor is not told (likelihood=None): None (= 'gaussian'), 'bernoulli' or 'dirichlet'.
# `--likelihood` of the evaluation drivers sets it (io_utils.parse_args('test')), for the same reason as amp: test_uncertainty.py does not pass the flag on.
likelihood = None

# objective of the DKT / DKTRegression models a process builds when their constructor is not told (objective=None): None (= 'mll', the marginal likelihood) or
# 'loo' (the leave-one-out predictive likelihood, docs/LOO.md; Gaussian likelihood only).  `--objective` of train.py / test.py sets it (io_utils.parse_args).
objective = None

save_dir = './save/'                     # checkpoints: <save_dir>checkpoints/<dataset>/<model>_<method>[_aug]_<n>way_<k>shot

# file-list roots of the image datasets (image_data.FilelistEpisodeLoader; `--dataset synthetic` needs none)
data_dir = {name: './filelists/%s/' % name for name in ('CUB', 'miniImagenet', 'omniglot', 'emnist')}
