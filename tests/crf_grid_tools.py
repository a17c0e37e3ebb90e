"""Host-side tools of the cvae_crf_grid tests (numpy, no GPU): the variant list that tests/test_gpu_crf_grid.py holds against
the float64 reference, and each variant's input probability.  tests/test_host_crf_grid.py qualifies the list on the CPU."""
import numpy as np

import segment_tools as st

KERNEL = st.WIDE_B[1:3] + st.WIDE_B[4:5]          # (alpha, beta, gamma) = (48, 40, 24)
IT = st.WIDE_B[5]

# (thr, p_floor, w1, w2).  thr -1: the soft prob1 of case_frames under (w1, w2, p_floor); the first is wideB itself.
# Thresholded variants read diff_u8 = trunc(prob1 * 255), which spans 12..242 on frames 0 and 1: 0 sets every pixel, 254 and
# 255 none (saturating thresholds), 127 about half.  A 0/1 input under the floor 1e-5 and the weights of wideB is decided by
# its unary alone (|u(0) - u(1)| = 11.5 against messages of at most 10) and never leaves Q(1) < 0.05 or > 0.95; the floor
# 0.3 (|u(0) - u(1)| = 1.2) with weights 0.6 / 0.4 keeps the mean field mid-range, so that the messages show in Q(1).
BASE_VARIANTS = (
    (-1, 1e-5, 6, 4),
    (-1, 1e-5, 0, 4),
    (-1, 1e-5, 6, 0),
    (-1, 1e-5, 0, 0),
    (-1, 1e-5, 3, 2),
    (-1, 0.5, 6, 4),
    (-1, 1e-30, 6, 4),
    (0, 0.3, 0.6, 0.4),
    (127, 0.3, 0.6, 0.4),
    (254, 0.3, 0.6, 0.4),
    (255, 0.3, 0.6, 0.4),
)
SATURATING = (0, 254, 255)


def variants(n):
    """BASE_VARIANTS repeated cyclically to n entries"""
    return [BASE_VARIANTS[i % len(BASE_VARIANTS)] for i in range(n)]


def diff_u8_of(prob1):
    return np.trunc(np.asarray(prob1, np.float32) * np.float32(255)).astype(np.uint8)


def variant_prob(variant, prob1, diff_u8):
    """the probability of label 1 that a variant's unary is built from, float32, shaped as prob1"""
    thr = variant[0]
    return np.asarray(prob1, np.float32) if thr < 0 else (np.asarray(diff_u8) > thr).astype(np.float32)


def variant_params(variant, it=IT):
    """(w1, alpha, beta, w2, gamma, it) of a variant under KERNEL, as crf_ref takes them"""
    _, _, w1, w2 = variant
    return (w1, KERNEL[0], KERNEL[1], w2, KERNEL[2], it)
