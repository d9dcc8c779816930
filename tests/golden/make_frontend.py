"""Makes ``tests/golden/frontend_pil.npz``: the reference's host chain on small images, recorded once.

    python tests/golden/make_frontend.py

Needs Pillow (the records name its version) and CPU torch.  Per shape of ``frontend_common.SHAPES``: a uniform-noise and a 0 / 255
input and Pillow's ``Image.resize((ow, oh), Image.BILINEAR)`` of both (what ``transforms.Resize`` calls, vfa/data/dataset.py:63);
for the shapes of ``TENSOR_SHAPES`` also ``ToTensor`` + ``(x - mean) / std`` (vfanet.py:59) of the noise output as float32, with the
model's constants and with (0, 1)."""
import os
import sys

import numpy as np
import torch
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frontend_common as fc  # noqa: E402


def to_tensor(pic):
    """torchvision's ``ToTensor`` for an 8-bit RGB image (functional.to_tensor: the bytes as CHW, ``.to(float32).div(255)``)."""
    try:
        from torchvision import transforms
        return transforms.ToTensor()(pic)
    except ImportError:
        return torch.from_numpy(np.asarray(pic).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def main():
    rng = np.random.default_rng(20240607)
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, shape in enumerate(fc.SHAPES):
        (ih, iw), (oh, ow) = shape
        inputs = {"noise": rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8),
                  "binary": (rng.integers(0, 2, (ih, iw, 3)) * 255).astype(np.uint8)}
        for name, a in inputs.items():
            pic = Image.fromarray(a).resize((ow, oh), Image.BILINEAR)
            out[fc.key(shape, name + "_in")] = a
            out[fc.key(shape, name + "_out")] = np.asarray(pic).copy()
            if i in fc.TENSOR_SHAPES and name == "noise":
                t = to_tensor(pic)
                for tag, mean, std in (("model", fc.MEAN, fc.STD), ("plain", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))):
                    m, s = torch.tensor(mean).view(3, 1, 1), torch.tensor(std).view(3, 1, 1)
                    out[fc.key(shape, "tensor_" + tag)] = ((t - m) / s).numpy()
    path = os.path.join(HERE, "frontend_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
