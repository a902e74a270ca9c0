"""RNN_ENCODER with cfg.RNN_TYPE 'GRU' (csrc/gru_mfma.hip, Fn.GruTrainFn) against
nn.Embedding weights + pack_padded_sequence + torch.nn.GRU + pad_packed_sequence in
float64 on the CPU: outputs and every parameter gradient by relative L2 error <= 1e-5,
the encoder's existing bound (test_gpu_lstm_train TOL, TOL_SENT).  torch.nn.GRU in
float32 against float64 on these inputs is at 2.2e-7 .. 2.5e-7 and no reference norm is
below 1.0, so the bound leaves about 40x over plain fp32 arithmetic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import rel_l2  # noqa: E402

T = 18
TOL = 1e-5
GRU_NAMES = [n + s for s in ('', '_reverse') for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]


def _captions(n, longest=T, seed=5):
    """Zero-padded captions over 50 tokens; the lengths walk through 1 .. longest."""
    g = torch.Generator().manual_seed(seed)
    lens = (7 * (torch.arange(n) + 5)) % longest + 1
    caps = torch.randint(1, 50, (n, T), generator=g)
    keep = (torch.rand((n, T, 300), generator=g) >= 0.5).to(torch.uint8)
    return caps * (torch.arange(T)[None, :] < lens[:, None]), lens, keep


def _ref(enc, caps, lens, Tout, keep=None, scale=2.0):
    """words, sent and the leaves {name: tensor} of the torch encoder in float64 on the CPU, enc's weights."""
    ref = torch.nn.GRU(enc.ninput, enc.nhidden, 1, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in enc.rnn.state_dict().items()})
    table = enc.encoder.weight.detach().cpu().double().requires_grad_()
    emb = table[caps]
    if keep is not None:
        emb = emb * keep.double() * scale
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, lens, batch_first=True, enforce_sorted=False)
    out, h_n = ref(packed)
    words = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=Tout)[0].transpose(1, 2)
    return words, h_n.transpose(0, 1).reshape(caps.shape[0], -1), dict(ref.named_parameters(), table=table)


def _encoder(gpu, drop_prob=0.5):
    """torch.nn.GRU's own default init under a seed, the embedding U(-0.1, 0.1)."""
    import DAMSM
    from miscc.config import cfg
    old, cfg.RNN_TYPE = cfg.RNN_TYPE, 'GRU'
    try:
        torch.manual_seed(41)
        return DAMSM.RNN_ENCODER(50, nhidden=256, drop_prob=drop_prob).to(gpu).train()
    finally:
        cfg.RNN_TYPE = old


def _grads(enc):
    return dict({n: getattr(enc.rnn, n).grad for n in GRU_NAMES}, table=enc.encoder.weight.grad)


@pytest.mark.parametrize('n,masked,longest', [(1, False, T), (1, True, T), (17, False, T), (17, True, T),
                                              (33, False, T), (33, True, T), (17, True, 11)])
def test_outputs_and_gradients_vs_fp64(gpu, n, masked, longest):
    enc = _encoder(gpu, 0.5 if masked else 0.0)
    caps, lens, keep = _captions(n, longest)
    assert n == 1 or (int(lens.min()) == 1 and int(lens.max()) == longest)
    keep = keep if masked else None
    g = torch.Generator().manual_seed(3)
    Gw, Gs = torch.randn((n, 256, longest), generator=g), torch.randn((n, 256), generator=g)
    words, sent = enc(caps.to(gpu), lens.to(gpu), max_len=longest, keep_mask=keep)
    assert words.grad_fn is not None
    ((words * Gw.to(gpu)).sum() + (sent * Gs.to(gpu)).sum()).backward()
    rw, rs, leaves = _ref(enc, caps, lens, longest, keep)
    ((rw * Gw.double()).sum() + (rs * Gs.double()).sum()).backward()
    errs = {'words': rel_l2(words, rw), 'sent': rel_l2(sent, rs)}
    got = _grads(enc)
    errs.update({k: rel_l2(got[k], v.grad) for k, v in leaves.items()})
    print('GRU n=%d masked=%d longest=%d rel_l2 vs fp64: %s'
          % (n, masked, longest, ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs
    absent = torch.ones(50, dtype=torch.bool)
    absent[caps.reshape(-1)] = False
    assert n > 1 or int(absent.sum()) >= 30
    assert not got['table'].cpu()[absent].any()      # exactly zero rows for the tokens not in the batch
    assert not words.detach().cpu().transpose(1, 2)[torch.arange(longest)[None, :] >= lens[:, None]].any()


@pytest.mark.parametrize('n,t', [(1, T), (17, T), (33, T), (2049, 6)])
def test_three_paths_same_bits(gpu, n, t):
    """eegan_gru_train_fwd on xproj rows gathered from the token table, encode_sentences (the
    table itself) and the frozen forward (its own x projections, the same dot products): one
    kernel body, so the same bits.  2049 captions are more 16-caption tiles than an MI355X has
    CUs: there the sentence launch is the 32-caption instantiation."""
    from eegan_hip._lib import ops
    from eegan_hip.tensor import stream, workspace
    H = 128
    enc = _encoder(gpu).eval()
    xtab, packed, bhn = enc._sent_tables()
    caps, lens, _ = _captions(n, t)
    caps = caps[:, :t].contiguous()
    ids, dlens = caps.to(gpu), lens.to(gpu)
    xproj = xtab[:, ids.reshape(-1)].contiguous()
    assert xproj.shape == (2, n * t, 3 * H)
    tape = workspace(ops.gru_train_workspace(n, t, H), gpu)
    hprev = torch.empty((2, n * t, H), device=gpu)
    words, sent = torch.empty((n, 2 * H, t), device=gpu), torch.empty((n, 2 * H), device=gpu)
    ops.gru_train_fwd(xproj.data_ptr(), packed.data_ptr(), bhn.data_ptr(), dlens.data_ptr(), n, t, H, t,
                      words.data_ptr(), sent.data_ptr(), tape.data_ptr(), hprev.data_ptr(), stream())
    batched = enc.encode_sentences(ids, dlens)
    with torch.no_grad():
        fwords, fsent = enc(ids, dlens, max_len=t)
    assert fwords.grad_fn is None
    assert torch.equal(sent, batched) and torch.equal(fsent, batched) and torch.equal(fwords, words)
    assert torch.equal(words[torch.arange(n, device=gpu), :H, dlens - 1], batched[:, :H])
    assert torch.equal(words[:, H:, 0], batched[:, H:])
    rw, rs, _ = _ref(enc, caps, lens, t)
    errs = rel_l2(fwords, rw), rel_l2(fsent, rs)
    print('GRU frozen n=%d rel_l2 vs fp64: words %.2e sent %.2e' % ((n,) + errs))
    assert max(errs) <= TOL, errs


def test_backward_is_deterministic(gpu):
    enc = _encoder(gpu)
    caps, lens, keep = _captions(33)
    g = torch.Generator().manual_seed(3)
    Gw, Gs = torch.randn((33, 256, T), generator=g).to(gpu), torch.randn((33, 256), generator=g).to(gpu)
    runs = []
    for _ in range(2):   # the second pass accumulates into the zeroed .grad tensors (Fn._grad_sink): 0 + x, the same bits
        enc.zero_grad(set_to_none=False)
        words, sent = enc(caps.to(gpu), lens.to(gpu), max_len=T, keep_mask=keep)
        ((words * Gw).sum() + (sent * Gs).sum()).backward()
        runs.append({k: v.clone() for k, v in _grads(enc).items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
