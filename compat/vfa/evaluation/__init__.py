"""``vfa.evaluation``: ``pyeval.evaluateAPAOS`` and ``pyeval.evaluateDetection`` come from the MI355X build; the rest of the reference's ``vfa/evaluation``
directory (evaluate.py, the MATLAB kit) is appended to the package path when it is present."""
import os

from .. import _reference_dirs

__path__ = [os.path.dirname(os.path.abspath(__file__))] + _reference_dirs("evaluation")
