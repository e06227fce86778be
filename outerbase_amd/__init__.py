"""outerbase_amd -- MI355X-native outer-product basis regression (hot path of
the R package outerbase) behind the reference's `obmod` module surface.

The arithmetic lives in libobhip.so (HIP kernels for gfx950 + C ABI declared in
include/obhip.h); this package is the host-side mirror of the reference's
Rcpp module (class and method names of src/interfaceR.cpp:661-793) plus the
obfit/obpred harness (R/fitting.R).  There is no CPU fallback.
"""
from . import _lib
from ._lib import ObhipError, device_count
from .obmod import (covf, covf_mat25, covf_mat25ang, covf_mat25pow, gethyp, getpara, hypnames,
                    listcov, loglik_gauss, loglik_gda, loglik_std, logpr_gauss, lpdf, lpdfvec,
                    outerbase, outermod, predict_grad, predict_hess, predict_hvp, predict_jac, predict_vjp,
                    predictor, setcovfs, setknot, term_dim_views)
from .fitting import BFGS_lpdf, BFGS_std, obfit, obpred, obpred_grad
from .multi import MultiFit, fit_newton_multi
from .glm import GlmFit, fit_glm
from .sensitivity import (ActiveSubspaceResult, ConditionalResult, GradMoments, InputMoments, ShapleyResult,
                          Sobol2Result, SobolResult, active_subspace, conditional_layout, conditional_moments,
                          conditional_tables, input_grad_moments, input_moments, interaction_effects, main_effects,
                          shapley, sobol, sobol2, sym_eigh, uniform_nodes)
from .design import AcquireGradResult, AcquireMultiResult, AcquireResult, DesignResult, Posterior, ThompsonResult
from .torch_emulator import TorchAcquisition, TorchCalibration, TorchEmulator
from .product import (CalibrationLoglik, fit_newton_product, predict_product, predict_product_grad,
                      product_fit_layout, product_grad_layout, product_layout, product_loglik, product_loglik_grad,
                      product_side)
from .driver import HotPath, MultiHotPath
from .stream import (CVResult, NewtonAccumulator, TermPathResult, cv_folds, cv_newton_multi, design_dx,
                     fit_newton_grad)

__all__ = [
    "ObhipError", "device_count", "covf", "covf_mat25", "covf_mat25ang", "covf_mat25pow", "gethyp",
    "getpara", "hypnames", "listcov", "loglik_gauss", "loglik_gda", "loglik_std", "logpr_gauss",
    "lpdf", "lpdfvec", "outerbase", "outermod", "predictor", "setcovfs", "setknot",
    "BFGS_lpdf", "BFGS_std", "obfit", "obpred",
    "MultiFit", "fit_newton_multi", "HotPath", "MultiHotPath",
    "NewtonAccumulator", "cv_newton_multi", "cv_folds", "CVResult",
    "predict_grad", "obpred_grad", "term_dim_views",
    "design_dx", "fit_newton_grad",
    "predict_jac", "predict_vjp", "predict_hvp", "predict_hess", "TorchEmulator",
    "GlmFit", "fit_glm",
    "Posterior", "DesignResult", "ThompsonResult", "AcquireResult", "AcquireGradResult", "TorchAcquisition",
    "InputMoments", "SobolResult", "input_moments", "uniform_nodes", "sobol", "main_effects",
    "Sobol2Result", "sobol2", "interaction_effects", "ShapleyResult", "shapley",
    "GradMoments", "ActiveSubspaceResult", "input_grad_moments", "active_subspace", "sym_eigh",
    "predict_product", "product_loglik", "product_layout", "CalibrationLoglik",
    "predict_product_grad", "product_loglik_grad", "product_grad_layout", "TorchCalibration",
    "fit_newton_product", "product_side", "product_fit_layout",
    "TermPathResult",
    "ConditionalResult", "conditional_layout", "conditional_moments", "conditional_tables",
    "AcquireMultiResult",
]
