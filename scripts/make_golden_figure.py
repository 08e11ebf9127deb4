#!/usr/bin/env python3
"""Generates tests/golden/figure_pillow_cases.npz: third-party known answers for the figure definition (include/thesia_amd.h,
"Export as figures").

A figure is Pillow's 16-bit Lanczos resize of a crop box (mode "I;16", `Image.resize((w, h), LANCZOS, box=...)`), with the box kept
in double where Pillow keeps it in float32: the cases of tests/figure_ref.py PILLOW_CASES use boxes that are exact in float32, so
the two agree bit for bit.  Inputs are closed-form integer images (tests/lod_images.py formulas: nothing to store); the fixture
holds Pillow's outputs only.

    python scripts/make_golden_figure.py          (needs Pillow; the tests do not)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.figure_ref import PILLOW_CASES, pillow_image  # noqa: E402


def pillow_resize(img: np.ndarray, out_w: int, out_h: int, box) -> np.ndarray:
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img, dtype=np.uint16))
    assert im.mode == "I;16", im.mode
    left, top, width, height = box
    r = im.resize((out_w, out_h), Image.LANCZOS, box=(left, top, left + width, top + height))
    out = np.asarray(r, dtype=np.uint16)
    assert out.shape == (out_h, out_w)
    return out


def main() -> None:
    import PIL
    data = {"pillow_version": np.array(PIL.__version__)}
    for k, (name, box, out_w, out_h) in enumerate(PILLOW_CASES):
        for v in box:
            assert float(np.float32(v)) == v and float(np.float32(box[0] + box[2])) == box[0] + box[2]
        data[f"case{k}"] = pillow_resize(pillow_image(name), out_w, out_h, box)
    out = os.path.join(ROOT, "tests", "golden", "figure_pillow_cases.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
