"""R-precision on the GPU: the batched sentence kernel (csrc/lstm_mfma.hip)
against torch.nn.LSTM in float64 on the CPU, the hit-scoring kernel
(csrc/rprec.hip) against float64 cosines, and metrics.r_precision_hits against
the reference-style one-by-one loop.

The encoder's bound is test_rnn_encoder's: relative L2 error <= 1e-5.  The
scores' bound is 5e-5 absolute: cosines lie in [-1, 1] and a 256-term fp32 dot
product is off by at most D * 2^-24 = 1.5e-5 in each of the three sums."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import golden, golden_state, fp, rel_l2  # noqa: E402
from oracle.seeding import seeded_state, seeded_tensor  # noqa: E402

T = 18
TOL_SENT = 1e-5
TOL_SCORE = 5e-5
# 4113 captions are more 16-caption tiles than an MI355X has CUs, so the launch takes the
# 32-caption kernel (with a partial last tile); the smaller sizes take the 16-caption one
BIG = 4113


def _encoder(gpu):
    import DAMSM
    enc = DAMSM.RNN_ENCODER(50, nhidden=256)
    enc.load_state_dict(golden_state('rnn', 41))
    return enc.to(gpu).eval()


def _captions(n, seed=5):
    """Zero-padded captions; the lengths start at T and walk through 1 .. T (1 at row 13)."""
    g = torch.Generator().manual_seed(seed)
    lens = (7 * (torch.arange(n) + 5)) % T + 1
    caps = torch.randint(1, 50, (n, T), generator=g)
    return caps * (torch.arange(T)[None, :] < lens[:, None]), lens


def _ref_sent(enc, caps, lens):
    """The sentence embedding of nn.Embedding + packed nn.LSTM in float64 with enc's weights."""
    ref = torch.nn.LSTM(enc.ninput, enc.nhidden, 1, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in enc.rnn.state_dict().items()})
    emb = enc.encoder.weight.detach().cpu().double()[caps]
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, lens, batch_first=True, enforce_sorted=False)
    with torch.no_grad():
        h_n = ref(packed)[1][0]
    return h_n.transpose(0, 1).reshape(caps.shape[0], -1)


@pytest.mark.parametrize('n', [1, 17, 33, BIG])
def test_encode_sentences_vs_fp64(gpu, n):
    enc = _encoder(gpu)
    caps, lens = _captions(n)
    assert n == 1 or (int(lens.min()) == 1 and int(lens.max()) == T)
    ref = _ref_sent(enc, caps, lens)
    new = rel_l2(enc.encode_sentences(caps.to(gpu), lens.to(gpu)), ref)
    old = rel_l2(enc(caps.to(gpu), lens.to(gpu))[1], ref)
    print('SENT n=%d rel_l2 vs fp64: batched %.3e, lstm_bidir %.3e' % (n, new, old))
    assert new <= TOL_SENT, new


def test_encode_sentences_golden(gpu):
    g = golden()
    enc = _encoder(gpu)
    caps = torch.as_tensor(g['rnn/caps']).long().reshape(4, 10).to(gpu)
    s = enc.encode_sentences(caps, torch.as_tensor(g['rnn/lens']).long().to(gpu))
    got, ref = np.asarray(fp(s.cpu()), np.float64).reshape(-1), np.asarray(g['rnn/sent'], np.float64).reshape(-1)
    assert got.shape == ref.shape
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) <= TOL_SENT


def test_encode_sentences_batch_independent(gpu):
    """Bitwise: a caption's embedding does not depend on its tile, its slot, its
    neighbours' lengths, or on which tile size the launch picked."""
    enc = _encoder(gpu)
    caps, lens = _captions(33)
    base = enc.encode_sentences(caps.to(gpu), lens.to(gpu))
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(1))
    more, more_lens = _captions(5, seed=6)
    s = enc.encode_sentences(torch.cat([caps[perm], more]).to(gpu), torch.cat([lens[perm], more_lens]).to(gpu))
    assert torch.equal(s[:33], base[perm.to(gpu)])
    big, big_lens = _captions(BIG - 33, seed=7)
    s = enc.encode_sentences(torch.cat([big, caps]).to(gpu), torch.cat([big_lens, lens]).to(gpu))
    assert torch.equal(s[BIG - 33:], base)


def _cos64(cnn, own, cand):
    rows = torch.cat([own[:, None], cand], 1).double()
    c = cnn.double()
    return (rows @ c[:, :, None])[..., 0] / (c.norm(dim=1, keepdim=True) * rows.norm(dim=2)).clamp(min=1e-8)


@pytest.mark.parametrize('B,R', [(1, 2), (5, 100)])
def test_rprec_hits_vs_fp64(gpu, B, R):
    from eegan_hip._lib import ops
    from eegan_hip.tensor import stream
    D = 256
    g = torch.Generator().manual_seed(1)   # fp64 top-two gaps of the unplanted rows: 3.5e-2 and 1.4e-2
    cnn, own, cand = (torch.randn(s, generator=g) for s in ((B, D), (B, D), (B, R - 1, D)))
    if B > 1:
        own[0] = 2 * cnn[0]
        cand[0, 7] = own[0]          # an exact tie with index 0: still a hit
        cand[1, R - 2] = 3 * cnn[1]  # the strict winner at the last index: a miss
    ref = _cos64(cnn, own, cand)
    top2 = ref[2 if B > 1 else 0:].topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3
    want = (ref.argmax(1) == 0).int()
    if B > 1:
        assert want[0] == 1 and want[1] == 0
    cd, od, xd = cnn.to(gpu), own.to(gpu), cand.to(gpu)
    scores = torch.empty((B, R), device=gpu)
    hits = torch.empty(B, dtype=torch.int32, device=gpu)
    ops.rprec_hits(cd.data_ptr(), od.data_ptr(), xd.data_ptr(), B, R, D, scores.data_ptr(), hits.data_ptr(), stream())
    err = float((scores.cpu().double() - ref).abs().max())
    print('RPREC B=%d R=%d max |score - fp64| = %.3e' % (B, R, err))
    assert err <= TOL_SCORE
    assert torch.equal(hits.cpu(), want)
    hits.zero_()
    ops.rprec_hits(cd.data_ptr(), od.data_ptr(), xd.data_ptr(), B, R, D, None, hits.data_ptr(), stream())
    assert torch.equal(hits.cpu(), want)


def test_r_precision_hits_end_to_end(gpu):
    """B = 3, R = 5 against the reference's loop (test.py:318-334) built from
    RNN_ENCODER.forward and torch ops: candidate order, own sentence at index 0."""
    import DAMSM
    from metrics import r_precision_hits
    B, R = 3, 5
    txt = _encoder(gpu)
    img = DAMSM.CNN_ENCODER(256)
    img.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in img.state_dict().items()], 71))
    img = img.to(gpu).eval()
    x = seeded_tensor('rprec:x', (B, 3, 64, 64), 1, 'uniform').to(gpu)
    caps, lens = _captions(B + B * (R - 1), seed=9)
    caps, lens = caps.to(gpu), lens.to(gpu)
    own = txt(caps[:B], lens[:B])[1]
    cand_caps, cand_lens = caps[B:].reshape(B, R - 1, T), lens[B:].reshape(B, R - 1)
    hits, scores = r_precision_hits(img, txt, x, own, cand_caps, cand_lens, return_scores=True)
    with torch.no_grad():
        code = img(x)[1]
        for b in range(B):
            rnn = torch.cat([own[b:b + 1], txt(cand_caps[b], cand_lens[b])[1]])
            ref = (code[b:b + 1] @ rnn.t()) / (code[b:b + 1].norm(dim=1, keepdim=True) @ rnn.norm(dim=1, keepdim=True).t()
                                              ).clamp(min=1e-8)
            assert float((scores[b] - ref[0]).abs().max()) <= TOL_SCORE
            assert int(hits[b]) == int(torch.argmax(ref) == 0)
    # a scoring text encoder of its own encodes the own captions too
    hits2, scores2 = r_precision_hits(img, txt, x, None, cand_caps, cand_lens, caps=caps[:B], cap_lens=lens[:B],
                                      return_scores=True)
    assert float((scores2 - scores).abs().max()) <= TOL_SCORE and torch.equal(hits2, hits)
