"""speaker-recognition_amd -- MI355X-native MFCC + diagonal-GMM scoring hot path.

The compute lives in ``lib/pygmm.so`` (HIP kernels for gfx950 behind the C ABI declared in
``include/pygmm_hip.h``); the modules here mirror the reference's Python surface for that
path: ``pygmm`` (src/gmm/python/pygmm.py), ``gmmset`` (src/testbench/gmmset.py),
``feature`` (src/feature/MFCC.py, utils.py, __init__.py), ``interface``
(src/gui/interface.py) and ``cli`` (src/speaker-recognition.py); ``jfa`` holds the front of
src/jfa/ (per-session Baum-Welch statistics against a UBM) by the reference's names; ``scorenorm``
normalises the score matrices of a verification run against impostor cohorts on the device
(Z, T, ZT, S and adaptive S-norm) and reports EER and minDCF; ``calibration`` turns those scores into log-likelihood ratios by
logistic regression on the device, fuses systems and reports Cllr, min Cllr and the actual DCF; ``ivector`` and ``plda`` are the i-vector leg: extraction by the
factor estimator's names, then whitening, WCCN, length normalisation, cosine scoring and Gaussian PLDA on the device.
"""
__version__ = "0.1.0"

from .scorenorm import (asnorm, eer, llr_matrix, min_dcf, normalise, select_cohort, snorm, tnorm, znorm,  # noqa: E402,F401
                        ztnorm)
