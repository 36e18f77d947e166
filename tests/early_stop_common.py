"""Shared helpers of the early-stop tests (option "early_stop", include/l2s.h): the reference's outputs masked by the reference's own lengths, and
sub-batches of the committed B = 32 stop golden (rows of a batch are independent, so a sub-batch of the golden batch is a valid case)."""
import numpy as np
import torch

POST_LAYERS, POST_KERNEL = 5, 5
MARGIN = POST_LAYERS * (POST_KERNEL // 2)        # a post-net frame j reads pre-post-net frames j - 10 .. j + 10

# the sub-batches of tests/golden/stop_lrw_b32.npz by largest length, and the end step E = min(S, max length + MARGIN) each gives at S = 300
SUB_BATCHES = ((27, 22, 37), (228, 28, 238), (286, 29, 296), (300, 32, 300))


def rows_upto(lengths, max_len):
    """Indices of the golden clips whose length is <= max_len, in batch order."""
    return [i for i, n in enumerate(lengths.tolist()) if n <= max_len]


def end_step(lengths, S):
    return min(S, int(max(lengths.tolist())) + MARGIN)


def masked_mel(mel_post, lengths):
    """where(j < len_b, mel_post[b, :, j], 0) for (B, 80, S)."""
    S = mel_post.shape[2]
    keep = torch.arange(S)[None, :] < lengths.reshape(-1, 1).cpu()
    return torch.where(keep[:, None, :], mel_post.cpu(), torch.zeros((), dtype=mel_post.dtype))


def masked_attn(attn, lengths):
    """where(j < len_b, attn[b, j, :], 0) for (B, S, T)."""
    S = attn.shape[1]
    keep = torch.arange(S)[None, :] < lengths.reshape(-1, 1).cpu()
    return torch.where(keep[:, :, None], attn.cpu(), torch.zeros((), dtype=attn.dtype))


def gumbel_rows(gumbel, idx, per_clip=4):
    """Rows 4b .. 4b + 3 of every clip b of `idx` (min_T(29) = 4 content slots per clip)."""
    rows = [per_clip * b + k for b in idx for k in range(per_clip)]
    return gumbel[rows]
