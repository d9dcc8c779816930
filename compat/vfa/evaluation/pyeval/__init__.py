"""``vfa.evaluation.pyeval``: `evaluateAPAOS` and `evaluateDetection` are the alias modules next to this file; every other module of
the reference's ``vfa/evaluation/pyeval`` directory (IoU.py, CLEAR_MOD_HUN.py, cuda_op/) still resolves to the checkout."""
import os

from ... import _reference_dirs

__path__ = [os.path.dirname(os.path.abspath(__file__))] + _reference_dirs(os.path.join("evaluation", "pyeval"))
