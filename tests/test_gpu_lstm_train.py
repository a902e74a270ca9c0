"""The trainable text encoder (csrc/lstm_mfma.hip, Fn.LstmTrainFn) against
nn.Embedding weights + pack_padded_sequence + torch.nn.LSTM + pad_packed_sequence
in float64 on the CPU: outputs and every parameter gradient by relative L2 error
<= 1e-5, the encoder's existing bound (test_rnn_encoder, TOL_SENT).  torch.nn.LSTM
in float32 against float64 on these inputs is at 1.2e-7 .. 3.7e-7, so the bound
leaves about 27x over plain fp32 arithmetic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import golden_state, rel_l2  # noqa: E402

T = 18
TOL = 1e-5
LSTM_NAMES = [n + s for s in ('', '_reverse') for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]


def _captions(n, longest=T, seed=5):
    """Zero-padded captions over 50 tokens; the lengths walk through 1 .. longest."""
    g = torch.Generator().manual_seed(seed)
    lens = (7 * (torch.arange(n) + 5)) % longest + 1
    caps = torch.randint(1, 50, (n, T), generator=g)
    keep = (torch.rand((n, T, 300), generator=g) >= 0.5).to(torch.uint8)
    return caps * (torch.arange(T)[None, :] < lens[:, None]), lens, keep


def _ref(enc, caps, lens, Tout, keep, scale, dtype=torch.float64):
    """words, sent and the leaves {name: tensor} of the torch encoder in `dtype` on the CPU, enc's weights."""
    ref = torch.nn.LSTM(enc.ninput, enc.nhidden, 1, batch_first=True, bidirectional=True).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in enc.rnn.state_dict().items()})
    table = enc.encoder.weight.detach().cpu().to(dtype).requires_grad_()
    emb = table[caps]
    if keep is not None:
        emb = emb * keep.to(dtype) * scale
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, lens, batch_first=True, enforce_sorted=False)
    out, (h_n, _) = ref(packed)
    words = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=Tout)[0].transpose(1, 2)
    leaves = dict(ref.named_parameters(), table=table)
    return words, h_n.transpose(0, 1).reshape(caps.shape[0], -1), leaves


def _encoder(gpu, drop_prob=0.5):
    import DAMSM
    enc = DAMSM.RNN_ENCODER(50, nhidden=256, drop_prob=drop_prob)
    enc.load_state_dict(golden_state('rnn', 41))
    return enc.to(gpu).train()


def _grads(enc):
    return dict({n: getattr(enc.rnn, n).grad for n in LSTM_NAMES}, table=enc.encoder.weight.grad)


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
    ((words * Gw.to(gpu)).sum() + (sent * Gs.to(gpu)).sum()).backward()
    rw, rs, leaves = _ref(enc, caps, lens, longest, keep, 2.0)
    ((rw * Gw.double()).sum() + (rs * Gs.double()).sum()).backward()
    errs = {'words': rel_l2(words, rw), 'sent': rel_l2(sent, rs)}
    got = _grads(enc)
    errs.update({k: rel_l2(got[k], v.grad) for k, v in leaves.items()})
    print('LSTM_TRAIN n=%d masked=%d longest=%d rel_l2 vs fp64: %s'
          % (n, masked, longest, ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs
    absent = torch.ones(50, dtype=torch.bool)
    absent[caps.reshape(-1)] = False
    assert n > 1 or int(absent.sum()) >= 30
    assert not got['table'].cpu()[absent].any()      # exactly zero rows for the tokens not in the batch
    assert not words.detach().cpu().transpose(1, 2)[torch.arange(longest)[None, :] >= lens[:, None]].any()


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


@pytest.mark.parametrize('n,t', [(1, T), (17, T), (33, T), (2049, 6)])
def test_tape_and_sentence_paths_same_bits(gpu, n, t):
    """eegan_lstm_train_fwd on xproj rows gathered from the token table against
    eegan_lstm_sent_batched on the table itself: one kernel body, so the same bits.
    2049 captions are more 16-caption tiles than an MI355X has CUs: there the
    sentence launch is the 32-caption instantiation."""
    from eegan_hip._lib import ops
    from eegan_hip.tensor import stream, workspace
    H = 128
    enc = _encoder(gpu)
    xtab, packed = enc._sent_tables()
    caps, lens, _ = _captions(n, t)
    ids, lens = caps[:, :t].contiguous().to(gpu), lens.to(gpu)
    xproj = xtab[:, ids.reshape(-1)].contiguous()
    assert xproj.shape == (2, n * t, 4 * H)
    tape = workspace(ops.lstm_train_workspace(n, t, H), gpu)
    hprev = torch.empty((2, n * t, H), device=gpu)
    words, sent = torch.empty((n, 2 * H, t), device=gpu), torch.empty((n, 2 * H), device=gpu)
    ops.lstm_train_fwd(xproj.data_ptr(), packed.data_ptr(), lens.data_ptr(), n, t, H, t, words.data_ptr(),
                       sent.data_ptr(), tape.data_ptr(), hprev.data_ptr(), stream())
    batched = torch.empty((n, 2 * H), device=gpu)
    ops.lstm_sent_batched(xtab.data_ptr(), packed.data_ptr(), ids.data_ptr(), lens.data_ptr(), n, t, H, enc.ntoken,
                          batched.data_ptr(), stream())
    assert torch.equal(sent, batched)
    last = words[torch.arange(n, device=gpu), :H, lens - 1]
    assert torch.equal(last, batched[:, :H])
    assert torch.equal(words[:, H:, 0], batched[:, H:])


def test_frozen_path_untouched(gpu):
    enc = _encoder(gpu, drop_prob=0.0)
    caps, lens, _ = _captions(17)
    caps, lens = caps.to(gpu), lens.to(gpu)
    with torch.no_grad():
        w_train, s_train = enc(caps, lens)
        w_eval, s_eval = enc.eval()(caps, lens)
    assert w_train.grad_fn is None and torch.equal(w_train, w_eval) and torch.equal(s_train, s_eval)
    words, sent = enc.train()(caps, lens)
    assert words.grad_fn is not None and sent.grad_fn is not None
    assert rel_l2(words, w_eval) <= TOL and rel_l2(sent, s_eval) <= TOL
    for p in enc.parameters():
        p.requires_grad = False
    assert enc(caps, lens)[1].grad_fn is None


def test_sent_loss_end_to_end(gpu):
    """miscc.DAMSM_losses.sent_loss on the tape path's sentence codes, B = 4.  The gradient of
    encoder.weight against oracle.sent_loss on the float64 LSTM; bound max(1e-5, 8 x the error
    of the same chain in float32 on the CPU against float64): measured 4.3e-7 against a float32
    error of 2.8e-7 (so the bound is 1e-5)."""
    from miscc.DAMSM_losses import sent_loss
    from oracle import eegan_oracle as O
    B = 4
    enc = _encoder(gpu)
    caps, lens, keep = _captions(B)
    code = torch.randn((B, 256), generator=torch.Generator().manual_seed(7))
    labels = torch.arange(B)
    sent = enc(caps.to(gpu), lens.to(gpu), keep_mask=keep)[1]
    l0, l1 = sent_loss(code.to(gpu), sent, labels.to(gpu), None, B)
    (l0 + l1).backward()
    for name, p in enc.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
    ref = {}
    for dtype in (torch.float64, torch.float32):
        _, rs, leaves = _ref(enc, caps, lens, int(lens.max()), keep, 2.0, dtype)
        sum(O.sent_loss(code.to(dtype), rs, labels, None, B)).backward()
        ref[dtype] = leaves['table'].grad
    err32 = rel_l2(ref[torch.float32], ref[torch.float64])
    err = rel_l2(enc.encoder.weight.grad, ref[torch.float64])
    print('LSTM_TRAIN sent_loss d(encoder.weight) rel_l2 vs fp64: %.2e (torch fp32 on the CPU: %.2e)' % (err, err32))
    assert err <= max(1e-5, 8 * err32), (err, err32)
