"""Plain restatement of sliding-window inference (include/cvk.h, cvk_window_merge; cvk.SlidingWindow) for the CPU and GPU tests: the
window grid as the loop of mmseg's mode='slide' writes it, brute-force counts, and the merge composed from torch's own fp32 CPU
operators in visiting order.  The kernel does the same IEEE additions in the same order and one division, so the GPU tests compare
bitwise against merge_fp32."""
import numpy as np
import torch


def grid(H, W, crop, stride):
    """[(y1, x1, y2, x2), ...] in visiting order: the loop of mmseg's EncoderDecoder.slide_inference, with the crop clipped to the image
    (mmseg pads a smaller image instead; padding is out of scope here)."""
    (h_crop, w_crop), (h_stride, w_stride) = crop, stride
    h_grids = max(H - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(W - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1 = h_idx * h_stride
            x1 = w_idx * w_stride
            y2 = min(y1 + h_crop, H)
            x2 = min(x1 + w_crop, W)
            y1 = max(y2 - h_crop, 0)
            x1 = max(x2 - w_crop, 0)
            out.append((y1, x1, y2, x2))
    return out


def windows(H, W, crop, stride):
    """[(y1, x1, hw, ww), ...] in visiting order."""
    return [(y1, x1, y2 - y1, x2 - x1) for y1, x1, y2, x2 in grid(H, W, crop, stride)]


def counts(H, W, crop, stride):
    """int64 [H, W] by brute force: one += 1 per window."""
    c = torch.zeros((H, W), dtype=torch.int64)
    for y1, x1, y2, x2 in grid(H, W, crop, stride):
        c[y1:y2, x1:x2] += 1
    return c


def argmax_first(x):
    """First maximum over dim 1, a NaN wins (numpy's argmax returns the first occurrence and treats NaN as the largest)."""
    return torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.int64))


def merge_fp32(window_logits, H, W, crop, stride):
    """(logits fp32 [N,C,H,W], pred int64 [N,H,W]) of the windows' logits (a list of fp32 [N,C,hw,ww] in visiting order): zeros,
    out[window] += l in visiting order, out / counts, first-maximum arg-max."""
    wins = grid(H, W, crop, stride)
    assert len(wins) == len(window_logits)
    N, C = window_logits[0].shape[:2]
    out = torch.zeros((N, C, H, W), dtype=torch.float32)
    for (y1, x1, y2, x2), l in zip(wins, window_logits):
        assert l.dtype == torch.float32 and tuple(l.shape) == (N, C, y2 - y1, x2 - x1)
        out[:, :, y1:y2, x1:x2] += l
    out = out / counts(H, W, crop, stride).to(torch.float32)
    return out, argmax_first(out)


# (H, W, crop, stride): image smaller than / equal to / one more than the crop, stride equal to the crop, stride 1, a last window pulled
# back by less than one stride, the CamVid-sized default, and sizes the GPU tests use
GRID_TABLE = [
    (5, 7, (8, 12), (3, 7)),            # H < hc, W < wc: a single clipped window
    (8, 12, (8, 12), (3, 7)),           # H == hc
    (9, 13, (8, 12), (3, 7)),           # H == hc + 1: the second window pulled back to offset 1
    (16, 24, (8, 12), (8, 12)),         # stride equal to the crop, exact tiling
    (17, 23, (8, 12), (8, 12)),         # stride equal to the crop, ragged last row / column
    (9, 10, (4, 4), (1, 1)),            # stride 1: counts reach 16
    (17, 23, (8, 12), (3, 7)),          # last window pulled back by less than one stride both ways (rows 0 3 6 9, columns 0 7 11)
    (16, 16, (8, 8), (5, 5)),           # ragged last window
    (5, 30, (8, 12), (3, 7)),           # clipped one way only
    (720, 960, (360, 480), (240, 320)),
    (360, 480, (360, 480), (240, 320)),
    (450, 600, (360, 480), (240, 320)),
    (40, 56, (32, 48), (8, 8)),
    (64, 96, (32, 64), (32, 32)),
]
