"""The footprint rule of the deferred P2 conv (roi_mark_kernel, roi_align.hip) against the oracle's RoIAlign: a box reads the 8 x 8 blocks
{lo, hi of every valid y sample} x {lo, hi of every valid x sample}.  Probe: a map that is zero except for NaN in one block -- RoIAlign's
output is NaN exactly when it reads that block (a tap of weight 0 still multiplies its value, so NaN * 0 shows a read as well)."""
import numpy as np
import torch

from oracle import mcgaze_oracle as orc


def footprint_blocks(box, H, W, stride, P=7, S=2):
    """The rule of roi_mark_kernel, in the oracle's per-axis arithmetic: set of (block row, block column)."""
    x1, y1, x2, y2 = [torch.tensor(v, dtype=torch.float32) for v in box]
    ss = torch.tensor(1.0 / stride, dtype=torch.float32)
    g = (torch.arange(P * S, dtype=torch.float32) + 0.5) / S
    hit = []
    for a1, a2, L in ((y1, y2, H), (x1, x2, W)):
        s0, e0 = a1 * ss - 0.5, a2 * ss - 0.5
        c = s0 + g * ((e0 - s0) / P)
        lo, hi, _, _, invalid = orc._bilinear_axis(c, L)
        ok = ~invalid
        hit.append(set((lo[ok] // 8).tolist()) | set((hi[ok] // 8).tolist()))
    return {(by, bx) for by in hit[0] for bx in hit[1]}


def read_blocks(box, H, W, stride):
    """Blocks whose NaN reaches the oracle's RoIAlign output."""
    rois = torch.tensor([[0.0] + list(box)], dtype=torch.float32)
    out = set()
    for by in range((H + 7) // 8):
        for bx in range((W + 7) // 8):
            feat = torch.zeros(1, 1, H, W)
            feat[0, 0, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = float('nan')
            if torch.isnan(orc.roi_align(feat, rois, 1.0 / stride)).any():
                out.add((by, bx))
    return out


def boxes(seed, n, size):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        cx, cy = rs.uniform(-0.2, 1.2, 2) * size
        w, h = np.exp(rs.uniform(np.log(2), np.log(size), 2))
        out.append((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))
    # degenerate, whole image, beyond every edge, one pixel at the far corner
    out += [(100.0, 80.0, 100.0, 120.0), (0.0, 0.0, size, size), (-50.0, -40.0, size + 30.0, size + 60.0), (size - 1.0, size - 1.0, size, size)]
    return out


def test_footprint_rule_matches_oracle_roi_align_p2():
    H = W = 56
    for box in boxes(0, 24, 224):
        assert footprint_blocks(box, H, W, 4) == read_blocks(box, H, W, 4), box


def test_footprint_rule_matches_oracle_roi_align_non_square():
    H, W = 64, 48
    for box in boxes(1, 12, 256):
        assert footprint_blocks(box, H, W, 4) == read_blocks(box, H, W, 4), box
