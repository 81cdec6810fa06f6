"""The bicubic fold's option pair on the calls test_gpu_interp.py does not reach: warp_interpolation = 2 with
warp_subpixel_bits = 5 is refused at the call by the files, mixed-size, hybrid, ranked and multi-device forms too, before any
file is read or frame aligned, in either order of setting; with the pair undone every one of them runs."""
import numpy as np
import pytest

from libstacker_rs_amd import (RANSAC, EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType, Stacker, synth)
from libstacker_rs_amd.api import INTER_CUBIC, INTER_LINEAR

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 50, 1e-4, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


def _write_ppm(path, frame):
    h, w, _ = frame.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(frame[..., ::-1]).tobytes())          # BGR in memory, RGB in the file


def test_the_subpixel_conflict_on_files_mixed_hybrid_ranked_and_multi_device_calls(tmp_path):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"f{i}.ppm"))
        _write_ppm(paths[-1], f)
    missing = [str(tmp_path / "absent.ppm")] * 3                               # the refusal comes before any file is read
    mixed = [frames[0], np.ascontiguousarray(frames[1][:80, :112]), frames[2]]
    st, multi = Stacker(0), Stacker(devices=[0, 0])
    try:
        calls = {"ecc_match_files": lambda s, p=paths: s.ecc_match_files(p, ECC),
                 "keypoint_match_files": lambda s, p=paths: s.keypoint_match_files(p, KP),
                 "hybrid_match_files": lambda s, p=paths: s.hybrid_match_files(p, KP, ECC),
                 "keypoint_match (mixed sizes)": lambda s: s.keypoint_match(mixed, KP),
                 "hybrid_match": lambda s: s.hybrid_match(frames, KP, ECC),
                 "ecc_match_ranked": lambda s: s.ecc_match_ranked(frames, ECC),
                 "keypoint_match_ranked": lambda s: s.keypoint_match_ranked(frames, KP)}
        for order in ((("warp_interpolation", INTER_CUBIC), ("warp_subpixel_bits", 5)),
                      (("warp_subpixel_bits", 5), ("warp_interpolation", INTER_CUBIC))):
            for s in (st, multi):
                try:
                    for name, v in order:
                        s.set_option(name, v)
                    for what, call in calls.items():
                        with pytest.raises(InvalidParams, match="warp_interpolation.*warp_subpixel_bits"):
                            call(s)
                    with pytest.raises(InvalidParams, match="warp_interpolation.*warp_subpixel_bits"):
                        s.ecc_match(frames, ECC)
                finally:
                    s.set_option("warp_subpixel_bits", 0)
                    s.set_option("warp_interpolation", INTER_LINEAR)
            try:
                for name, v in order:
                    st.set_option(name, v)
                for what in ("ecc_match_files", "keypoint_match_files", "hybrid_match_files"):
                    # (the Python wrapper asks the first file's geometry itself, so the first path exists)
                    with pytest.raises(InvalidParams, match="warp_interpolation.*warp_subpixel_bits"):
                        calls[what](st, [paths[0]] + missing[1:])
            finally:
                st.set_option("warp_subpixel_bits", 0)
                st.set_option("warp_interpolation", INTER_LINEAR)
        for s in (st, multi):
            for call in calls.values():
                call(s)
    finally:
        st.close()
        multi.close()
