"""Alias of the reference's ``vfa/evaluation/pyeval/evaluateDetection.py``: ``evaluateDetection_py(res_fpath, gt_fpath, dataset_name)``
binds to the HIP build of the MODA / MODP evaluation -- same arguments, same ``(recall, precision, MODA, MODP)`` -- which computes the
distances and the Hungarian assignment of every frame in one launch instead of one scipy call per frame.  ``CLEAR_MOD_HUN.py`` itself
is not aliased: it still resolves to the checkout."""
from vfa_amd.eval_ops import evaluate_detection as evaluateDetection_py

__all__ = ["evaluateDetection_py"]
