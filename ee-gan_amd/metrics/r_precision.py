"""R-precision (reference test.py:306-357) on the HIP kernels.

The reference takes every generated image in turn: it draws R-1 captions of
other classes (`dataset.get_sent_multi_unpair`), runs the text encoder on
them, takes the cosine of the image code against [own sentence; candidates]
and counts a hit when index 0 wins.  Here a batch of B images is one image
encoder call, ONE text encoder call over all B*(R-1) candidates
(`RNN_ENCODER.encode_sentences`: the batched MFMA sentence kernel) and one
scoring launch (`eegan_rprec_hits`: one wave per image); nothing is read back
to the host until the caller looks at `hits`.
"""
import numpy as np
import torch

from eegan_hip._lib import ops
from eegan_hip.tensor import stream, F32


def r_precision_hits(image_encoder, text_encoder, fake_imgs, sent_emb, cand_caps, cand_lens, caps=None,
                     cap_lens=None, return_scores=False):
    """hits (B,) int32 on the device: 1 where the image's own sentence scores
    at least as high as each of its R-1 candidates (test.py:333, torch.argmax
    == 0).

    fake_imgs (B, 3, h, w); sent_emb (B, D): the own sentences as the
    generator's text encoder gave them; cand_caps (B, R-1, T) int64 and
    cand_lens (B, R-1): every image's candidates in drawing order.  When
    `text_encoder` is not the generator's (test.py:309-313) pass the own
    captions `caps` (B, T) / `cap_lens` (B,): they are encoded with
    `text_encoder` too and `sent_emb` is not used.  return_scores: also the
    cosines (B, R), index 0 the own sentence."""
    B, Rm1, T = cand_caps.shape
    with torch.no_grad():
        _, cnn_code = image_encoder(fake_imgs)
        cnn_code = cnn_code.detach().float().contiguous()
        dev = cnn_code.device
        cand = text_encoder.encode_sentences(cand_caps.reshape(B * Rm1, T), cand_lens.reshape(B * Rm1))
        own = sent_emb if caps is None else text_encoder.encode_sentences(caps, cap_lens)
        own = own.detach().to(dev).float().contiguous()
        cand = cand.to(dev).contiguous()
    D = cnn_code.shape[1]
    if cnn_code.shape[0] != B or tuple(own.shape) != (B, D) or cand.shape[1] != D:
        raise ValueError('r_precision_hits: image codes %s, own sentences %s, candidates %s for B=%d'
                         % (tuple(cnn_code.shape), tuple(own.shape), tuple(cand.shape), B))
    hits = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty((B, Rm1 + 1), dtype=F32, device=dev) if return_scores else None
    ops.rprec_hits(cnn_code.data_ptr(), own.data_ptr(), cand.data_ptr(), B, Rm1 + 1, D,
                   scores.data_ptr() if return_scores else None, hits.data_ptr(), stream())
    return (hits, scores) if return_scores else hits


def r_precision_mean_std(hits, real_sampling_nums, clusters=10):
    """test.py:339-357 (cal_sim_mean_std) as written: the hits are shuffled in
    place with numpy's global generator, cut into `clusters` runs of
    min(real_sampling_nums, 30000) // clusters, and the mean / std taken over
    the runs' averages.  The reference's slice [st : ed] with
    ed = (ix + 1) * n - 1 leaves the last element of every run out; that
    changes the number, so it is kept."""
    n = min(real_sampling_nums, 30000) // clusters
    np.random.shuffle(hits)
    runs = np.array([np.average(hits[k * n: (k + 1) * n - 1]) for k in range(clusters)])
    return np.average(runs), np.std(runs)
