"""Writes tests/golden/bev_image_recorded_run.npz from a run the reference recorded itself: the
bytes of the camera frame it read (kuruma/test/raw_collected_data/raw_images/STEM.jpg, 640 x 360)
and of the bird's-eye picture it wrote for it (kuruma/test/output/STEM_bird_eye.jpg, 208 x 108:
corrected calibration, 1 pixel per cm, margin 0.1, full image), each as a uint8 array of the
file's bytes.  tests/test_bev_image_cpu.py decodes both.

    python tools/gen_bev_image_golden.py REFERENCE/kuruma/test [raw_20250702_024355_405]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(test_dir, stem="raw_20250702_024355_405"):
    src = os.path.join(test_dir, "raw_collected_data", "raw_images", stem + ".jpg")
    out = os.path.join(test_dir, "output", stem + "_bird_eye.jpg")
    np.savez(os.path.join(ROOT, "tests", "golden", "bev_image_recorded_run.npz"),
             source_jpeg=np.fromfile(src, dtype=np.uint8),
             bird_eye_jpeg=np.fromfile(out, dtype=np.uint8),
             source=np.array(stem))


if __name__ == "__main__":
    main(*sys.argv[1:])
