"""TEST INFRASTRUCTURE ONLY -- the cases that tests/test_skip_absent_emul.py (the host-compiled kernel) and
tests/test_skip_absent_gpu.py (the device) both hold to hostglue.present_rows, and a plain-loop reference of the compaction
written from the text of include/emo_hip.h (ABI 27) alone: Python ints, no numpy arithmetic, nothing imported from
emoportraits_amd."""
import numpy as np

FILL = 0x5A5A5A5A                      # what the outputs hold before a launch that must overwrite every element


def reference(crop, paste, F, P):
    """the header's text as loops -> (count [F], first [F + 1], row_of [M], crop_out [M,4], paste_out [M,4]), int32"""
    M = F * P
    count, first = np.zeros((F,), np.int32), np.zeros((F + 1,), np.int32)
    row_of = np.full((M,), -1, np.int32)
    crop_out, paste_out = np.zeros((M, 4), np.int32), np.zeros((M, 4), np.int32)
    j = 0
    for i in range(M):
        if i % P == 0:
            first[i // P] = j
        if int(paste[i][2]) > 0:
            row_of[j] = i
            for c in range(4):
                crop_out[j][c] = crop[i][c]
                paste_out[j][c] = paste[i][c]
            j += 1
    first[F] = j
    for f in range(F):
        count[f] = int(first[f + 1]) - int(first[f])
    return count, first, row_of, crop_out, paste_out


def windows(present, seed=0):
    """crop and paste [M,4] int32 as the tracker writes them for the rows `present` (flat, frame-major): a present row has one
    window of its own in both, an absent one a centred square to read and (0, 0, 0, 0) to paste"""
    rng = np.random.default_rng(seed)
    present = np.asarray(present, bool).reshape(-1)
    M = present.shape[0]
    crop = np.empty((M, 4), np.int32)
    crop[:, 0], crop[:, 1] = rng.integers(0, 400, M), rng.integers(0, 300, M)
    crop[:, 2] = crop[:, 3] = 2 * rng.integers(1, 200, M)
    paste = crop.copy()
    crop[~present] = (420, 0, 1080, 1080)
    paste[~present] = 0
    return crop, paste


def cases():
    """name -> (crop, paste, F, P)"""
    rng = np.random.default_rng(27)
    out = {
        "one_present": (*windows([1]), 1, 1),
        "one_absent": (*windows([0]), 1, 1),
        "all_absent": (*windows(np.zeros(12)), 4, 3),
        "all_present": (*windows(np.ones(12)), 4, 3),
        # frames 1 and 3 are empty
        "mixed_5x3": (*windows([1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1], 1), 5, 3),
        "sixteen_tracks": (*windows(rng.random(7 * 16) < 0.4, 2), 7, 16),
    }
    for M, P in ((255, 1), (256, 2), (257, 1), (1120, 2)):      # uneven runs; threads behind the last row
        out[f"rows_{M}"] = (*windows(rng.random(M) < 0.6, M), M // P, P)
    # absent by a negative side, and by a side of 0 beside a non-zero x / y
    crop, paste = windows(np.ones(8), 3)
    paste[1] = (5, 7, -4, -4)
    paste[2] = (9, 11, 0, 0)
    paste[6] = (0, 3, 0, 12)
    out["odd_absent"] = (crop, paste, 4, 2)
    return out


def prefilled(F, P):
    """the five outputs holding FILL in every element"""
    M = F * P
    return [np.full(shape, FILL, np.int32) for shape in ((F,), (F + 1,), (M,), (M, 4), (M, 4))]
