"""Alias of the reference's ``vfa/evaluation/pyeval/evaluateAPAOS.py``: ``evaluate.py:3`` (``from vfa.evaluation.pyeval.evaluateAPAOS
import evaluateDetectionAPAOS``) binds to the HIP build of the metric -- same two file arguments, same 9-tuple -- which computes all
the rotated-box IoUs of the evaluation set in one launch instead of one host round trip per (detection, ground truth) pair."""
from vfa_amd.eval_ops import evaluate_ap_aos as evaluateDetectionAPAOS

__all__ = ["evaluateDetectionAPAOS"]
