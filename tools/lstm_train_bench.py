"""Forward + backward of the trainable text encoder (RNN_ENCODER with gradients
wanted: Fn.LstmTrainFn, csrc/lstm_mfma.hip; with --rnn GRU Fn.GruTrainFn,
csrc/gru_mfma.hip), event-timed:

    python tools/lstm_train_bench.py [--rnn LSTM|GRU|both] [--batch 48] [--words 18] [--vocab 5450]
                                     [--cands 1584] [--repeats 7] [--iters 20] [--out FILE]

  whole        train-mode forward (dropout mask drawn) + backward of
               (words * Gw).sum() + (sent * Gs).sum() into every parameter;
  forward      the tape path's forward alone;
  frozen       the no-grad forward (LSTM: lstm_seq_kernel; GRU: eegan_gru_fwd), for scale;
  fwd kernel / bwd kernel
               eegan_{lstm,gru}_train_fwd / _bwd alone on the same shapes, back
               to back launches;
  sentences    encode_sentences of --cands captions in eval mode (R-precision's
               text side at tools/rprec_bench.py's shape: 16 x 99 candidates).

Windows of `iters` calls, the ways alternating (with --rnn both, the two
encoders' ways in one session); medians over `repeats` windows with min and max.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'ee-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def ways_of(rnn, a, dev):
    """[(name, callable)] for one encoder type."""
    import DAMSM
    from miscc.config import cfg
    from eegan_hip import functional as Fn
    from eegan_hip._lib import ops
    from eegan_hip.tensor import stream, workspace
    N, T, H = a.batch, a.words, 128
    gates = 4 if rnn == 'LSTM' else 3
    old, cfg.RNN_TYPE = cfg.RNN_TYPE, rnn
    try:
        enc = DAMSM.RNN_ENCODER(a.vocab, nhidden=2 * H).to(dev).train()
        sen = DAMSM.RNN_ENCODER(a.vocab, nhidden=2 * H).to(dev).eval()
    finally:
        cfg.RNN_TYPE = old
    lens = torch.randint(5, T + 1, (N,), device=dev)
    lens[0] = T
    caps = torch.randint(1, a.vocab, (N, T), device=dev) * (torch.arange(T, device=dev)[None, :] < lens[:, None])
    Gw, Gs = torch.randn(N, 2 * H, T, device=dev), torch.randn(N, 2 * H, device=dev)
    clens = torch.randint(5, T + 1, (a.cands,), device=dev)
    ccaps = torch.randint(1, a.vocab, (a.cands, T), device=dev) * (torch.arange(T, device=dev)[None, :] < clens[:, None])

    def whole():
        words, sent = enc(caps, lens, max_len=T)
        ((words * Gw).sum() + (sent * Gs).sum()).backward()

    def frozen():
        with torch.no_grad():
            enc(caps, lens, max_len=T)

    # the two recurrence kernels on buffers of their own
    whh = torch.stack([enc.rnn.weight_hh_l0.detach(), enc.rnn.weight_hh_l0_reverse.detach()])
    pf, pb = Fn.pack_whh_fwd(whh.transpose(1, 2), gates), Fn.pack_whh_bwd(whh)
    xproj = torch.randn(2, N * T, gates * H, device=dev)
    bhn = torch.randn(2, H, device=dev)
    tape = workspace(getattr(ops, rnn.lower() + '_train_workspace')(N, T, H), dev)
    hprev, dxproj = torch.empty(2, N * T, H, device=dev), torch.empty(2, N * T, gates * H, device=dev)
    dhn = torch.empty(2, N * T, H, device=dev)
    words, sent = torch.empty(N, 2 * H, T, device=dev), torch.empty(N, 2 * H, device=dev)

    if rnn == 'LSTM':
        def fwd_kernel():
            ops.lstm_train_fwd(xproj.data_ptr(), pf.data_ptr(), lens.data_ptr(), N, T, H, T, words.data_ptr(),
                               sent.data_ptr(), tape.data_ptr(), hprev.data_ptr(), stream())

        def bwd_kernel():
            ops.lstm_train_bwd(Gw.data_ptr(), Gs.data_ptr(), pb.data_ptr(), lens.data_ptr(), tape.data_ptr(), N, T, H,
                               T, dxproj.data_ptr(), stream())
    else:
        def fwd_kernel():
            ops.gru_train_fwd(xproj.data_ptr(), pf.data_ptr(), bhn.data_ptr(), lens.data_ptr(), N, T, H, T,
                              words.data_ptr(), sent.data_ptr(), tape.data_ptr(), hprev.data_ptr(), stream())

        def bwd_kernel():
            ops.gru_train_bwd(Gw.data_ptr(), Gs.data_ptr(), pb.data_ptr(), lens.data_ptr(), tape.data_ptr(),
                              hprev.data_ptr(), N, T, H, T, dxproj.data_ptr(), dhn.data_ptr(), stream())

    fwd_kernel()   # the bwd kernel reads a tape the fwd kernel wrote
    return [('whole', whole), ('forward', lambda: enc(caps, lens, max_len=T)), ('frozen', frozen),
            ('fwd kernel', fwd_kernel), ('bwd kernel', bwd_kernel),
            ('sentences', lambda: sen.encode_sentences(ccaps, clens))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rnn', choices=['LSTM', 'GRU', 'both'], default='LSTM')
    ap.add_argument('--batch', type=int, default=48)
    ap.add_argument('--words', type=int, default=18)
    ap.add_argument('--vocab', type=int, default=5450)
    ap.add_argument('--cands', type=int, default=1584)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lstm_train_bench needs a HIP device')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    ways = []
    for rnn in (['LSTM', 'GRU'] if a.rnn == 'both' else [a.rnn]):
        ways += [('%s %s' % (rnn, name), f) for name, f in ways_of(rnn, a, dev)]
    for _ in range(3):   # warm-up: code objects, the allocator's blocks
        for _, f in ways:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in ways]
    for _ in range(a.repeats):
        for k, (_, f) in enumerate(ways):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.iters)
    lines = ['N=%d T=%d vocab=%d E=300 H=128, sentences: %d captions: %d windows of %d calls, the ways alternating; '
             'longest caption %d steps' % (a.batch, a.words, a.vocab, a.cands, a.repeats, a.iters, a.words)]
    for (name, _), m in zip(ways, ms):
        m.sort()
        lines.append('%-16s median %.3f ms per call (min %.3f, max %.3f)' % (name, m[len(m) // 2], m[0], m[-1]))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
