#!/usr/bin/env python3
"""Generates tests/golden/jpeg_v1.npz — JPEG files written by Pillow, and Pillow's own decode of them, for
tests/test_cpu_host.py::test_imread_jpeg_through_runtime_libjpeg (the engine's decoder against a second decoder family).

The picture is a 123 x 211 gradient with a red block (`host_src` below; the test computes it the same way). Four
encodings: 4:4:4 quality 92, 4:2:0 quality 85, progressive 4:4:4 quality 85, and the red channel alone as grey, quality
90. They were written with Pillow 8.4 on IJG libjpeg 9. Pillow's decode of each file read by the test is stored as its
difference from the source picture (int8), which keeps the file small. Run from the repo root, naming an interpreter
that has Pillow and numpy:
    python tests/golden/make_jpeg.py --pillow-python /path/to/python3

Entries: host_{c444,c420,prog,grey}_jpg (1-D uint8: the file's bytes), host_{c444,prog,grey}_minus_src (int8).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

PILLOW_CODE = """
import sys
import numpy as np
from PIL import Image
d = sys.argv[1]
h, w = 123, 211
yy, xx = np.mgrid[0:h, 0:w]
img = np.stack([xx * 255 // w, yy * 255 // h, (xx + yy) * 3 % 256], -1).astype(np.uint8)
img[30:60, 40:90] = [250, 10, 30]
Image.fromarray(img).save(d + '/c444.jpg', quality=92, subsampling=0)
Image.fromarray(img).save(d + '/c420.jpg', quality=85, subsampling=2)
Image.fromarray(img).save(d + '/prog.jpg', quality=85, progressive=True, subsampling=0)
Image.fromarray(img[..., 0]).save(d + '/grey.jpg', quality=90)
for n in ('c444', 'prog', 'grey'):
    np.save(d + '/' + n + '.npy', np.asarray(Image.open(d + '/' + n + '.jpg')))
"""


def host_src():
    """The picture the four files encode (RGB, as Pillow was given it)."""
    h, w = 123, 211
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // w, yy * 255 // h, (xx + yy) * 3 % 256], -1).astype(np.uint8)
    img[30:60, 40:90] = [250, 10, 30]
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pillow-python", default=sys.executable, help="interpreter with Pillow and numpy")
    args = ap.parse_args()
    out = {}
    src = host_src().astype(np.int16)
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([args.pillow_python, "-c", PILLOW_CODE, d], check=True)
        for n in ("c444", "c420", "prog", "grey"):
            out["host_%s_jpg" % n] = np.fromfile(os.path.join(d, n + ".jpg"), np.uint8)
        for n in ("c444", "prog", "grey"):
            diff = np.load(os.path.join(d, n + ".npy")).astype(np.int16) - (src[..., 0] if n == "grey" else src)
            assert np.abs(diff).max() <= 127
            out["host_%s_minus_src" % n] = diff.astype(np.int8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes:", ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
