#!/usr/bin/env python3
"""tools/make_center_head_nms_wide.py -- tests/golden/center_head_nms_wide.npz: the boxes [5, 1024, 7] fp32 of the "wide" NMS case of
tests/center_head_cases.py (counts 1024, 1023, 961, 960, 0; 16 mask words).  Drawing them takes about 6 s (every box is redrawn while an
fp64 IoU with an earlier box lies within 0.02 of the threshold), so the suite loads the fixture; the IoU matrices are recomputed on load.

    python tools/make_center_head_nms_wide.py          # rewrites the fixture (140 KiB)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import center_head_cases as CC  # noqa: E402

if __name__ == "__main__":
    boxes, counts, ious = CC.nms_edge_generate("wide")
    thresh, _, _, margin, _ = CC.NMS_EDGE_CASES["wide"]
    for g, n in enumerate(counts):
        assert CC.greedy_nms(boxes[g, :n], thresh, 10 ** 6, 10 ** 6, ious[g])[1] >= margin
    path = os.path.join(ROOT, "tests", "golden", CC.NMS_WIDE_GOLDEN)
    np.savez_compressed(path, boxes=boxes)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")
