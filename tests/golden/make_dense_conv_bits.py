"""Makes ``tests/golden/dense_conv_bits_parent.json``: the output bits of the heads' and the trunk's dense convolutions, recorded once.

    python tests/golden/make_dense_conv_bits.py

Needs the MI355X and the built library.  It was run on the commit BEFORE the two kernels were folded into one template
(vfa_amd/csrc/vfa_dense.h); tests/test_dense_conv_bits.py holds every later commit to these bits.  Per case of
tests/dense_bits_common.py: the output's shape and the SHA-256 of its contiguous float32 bytes; the ``hipcc --version`` line of the
build is recorded for information.  Only public ``ops`` calls on seeded CPU generators."""
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dense_bits_common as db  # noqa: E402


def hipcc_version():
    try:
        lines = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()
        return next((l.strip() for l in lines if "HIP version" in l), lines[0].strip() if lines else "unknown")
    except OSError:
        return "unknown"


def main():
    dev = torch.device("cuda:0")
    out = {"hipcc": hipcc_version(), "cases": {}}
    for name in db.NAMES:
        y = db.compute(name, dev)
        assert float(y.abs().max()) > 0 and bool(torch.isfinite(y).all()), name
        out["cases"][name] = {"shape": list(y.shape), "sha256": db.digest(y)}
        print(name, out["cases"][name])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dense_conv_bits_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
