"""fp64 restatement of the test-time-augmentation merge (include/cvk.h, cvk_tta_accumulate / cvk_tta_resize_input; cvk.TestTimeAugmentation),
written from its definition for the CPU and GPU tests: integer-weight bilinear resampling, softmax, flip, the ordered sum and the
first-maximum arg-max.  Also the yardstick the tolerances come from: the same merge composed from torch's own fp32 CPU operators."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def taps(out, inn):
    """Bilinear taps of `out` destination samples over `inn` source samples (align_corners=False) from integers:
    (lower index, upper index, lower weight, upper weight), the weights as exact fp64 quotients."""
    d = np.arange(out, dtype=np.int64)
    num = np.maximum((2 * d + 1) * inn - out, 0)
    den = 2 * out
    i0 = num // den
    i1 = np.minimum(i0 + 1, inn - 1)
    f = (num % den).astype(np.float64) / float(den)
    return i0, i1, 1.0 - f, f


def resize(x, H, W):
    """[N,C,h,w] -> fp64 [N,C,H,W]: wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d)."""
    x = torch.as_tensor(x).double()
    y0, y1, wy0, wy1 = taps(H, x.shape[2])
    x0, x1, wx0, wx1 = taps(W, x.shape[3])
    wx0, wx1 = torch.from_numpy(wx0), torch.from_numpy(wx1)
    wy0, wy1 = torch.from_numpy(wy0)[:, None], torch.from_numpy(wy1)[:, None]
    top, bot = x[:, :, y0, :], x[:, :, y1, :]
    return wy0 * (wx0 * top[..., x0] + wx1 * top[..., x1]) + wy1 * (wx0 * bot[..., x0] + wx1 * bot[..., x1])


def softmax(x):
    x = x.double()
    e = torch.exp(x - x.amax(dim=1, keepdim=True))
    return e / e.sum(dim=1, keepdim=True)


def argmax_first(p):
    """First maximum over dim 1 (numpy's argmax returns the first occurrence)."""
    return torch.from_numpy(np.argmax(p.numpy(), axis=1).astype(np.int64))


def view_probs(logits, flipped, H, W):
    p = softmax(resize(logits, H, W))
    return p.flip(-1) if flipped else p


def merge(logits, flips, H, W):
    """(probs fp64 [N,C,H,W], pred int64 [N,H,W]) of the views' logits (a list of [N,C,h,w]) and their mirrored flags."""
    acc = None
    for lg, fl in zip(logits, flips):
        p = view_probs(lg, fl, H, W)
        acc = p if acc is None else acc + p
    probs = acc * (1.0 / len(logits))
    return probs, argmax_first(probs)


def input_view(images, h, w, flipped):
    """The network input of one view, fp64."""
    v = resize(images, h, w)
    return v.flip(-1) if flipped else v


def view_sizes(H, W, scales, flip, size_divisor=1):
    out = []
    for s in scales:
        h = size_divisor * math.ceil(math.floor(H * s + 0.5) / size_divisor)
        w = size_divisor * math.ceil(math.floor(W * s + 0.5) / size_divisor)
        out.append((h, w, False))
        if flip:
            out.append((h, w, True))
    return out


def torch_fp32_merge(logits, flips, H, W):
    """The yardstick: the merge composed from torch's fp32 CPU operators (interpolate, softmax, flip, ordered sum, * float32(1/K))."""
    acc = None
    for lg, fl in zip(logits, flips):
        up = F.interpolate(lg.float(), (H, W), mode="bilinear", align_corners=False)
        p = torch.softmax(up, dim=1)
        p = p.flip(-1) if fl else p
        acc = p if acc is None else acc + p
    return acc * torch.tensor(np.float32(1.0) / np.float32(len(logits)))


def yardstick(logits, flips, H, W):
    """Largest deviation of torch's fp32 composition from the restatement on these inputs."""
    return float((torch_fp32_merge(logits, flips, H, W).double() - merge(logits, flips, H, W)[0]).abs().max())


def near_ties(probs, gap):
    """bool [N,H,W]: pixels whose two largest mean probabilities differ by less than `gap`."""
    top = probs.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < gap


def tolerance(yard):
    """4x the yardstick (the margin this project gives over a reference's own drift), never more than the 1e-5 the losses are held to."""
    return min(4.0 * yard, 1e-5)


def draw_views(seed, N, C, sources):
    """Seeded logits 3 * randn, one map per source size, each used unflipped and then mirrored as its own draw: six views for three sizes."""
    g = torch.Generator().manual_seed(seed)
    logits, flips = [], []
    for h, w in sources:
        for fl in (False, True):
            logits.append(3.0 * torch.randn((N, C, h, w), generator=g))
            flips.append(fl)
    return logits, flips


# the C-ABI cases of tests/test_gpu_tta.py: name -> (seed, N, C, (H, W), sources, ld)
CASES = {
    "c12_17x23": (0, 2, 12, (17, 23), ((12, 16), (17, 23), (23, 31)), 12),       # odd sizes, 782 pixels: up, identity, down
    "c12_17x23_ld16": (0, 2, 12, (17, 23), ((12, 16), (17, 23), (23, 31)), 16),  # padded pixel stride
    "c5_16x16": (1, 1, 5, (16, 16), ((8, 8), (16, 16), (33, 29)), 5),            # general-C path
    "c21_16x16": (2, 1, 21, (16, 16), ((8, 8), (16, 16), (33, 29)), 21),         # a swapped head
    "c12_45x60": (3, 2, 12, (45, 60), ((34, 45), (45, 60), (56, 75)), 12),       # several workgroups with a tail
}
