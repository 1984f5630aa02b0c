"""Evaluation metrics (reference: metrics/), computed by HIP kernels."""
from .any_size import masked_ms_ssim_any, ms_ssim_any  # noqa: F401
