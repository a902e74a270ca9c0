"""R-precision for one evaluation batch, two ways, in one process:

  (a) the loop of test.py:318-334 on the existing kernels: per image one
      RNN_ENCODER.forward on its R-1 candidates, then torch scoring;
  (b) metrics.r_precision_hits: one batched sentence-kernel launch over all
      B*(R-1) candidates (csrc/lstm_mfma.hip) and one scoring launch
      (csrc/rprec.hip).

    python tools/rprec_bench.py [--batch 16] [--r 100] [--words 18] [--vocab 5450] [--repeats 7] [--iters 10] [--out FILE]

Both are timed with and without the image encoder call they share ("whole" /
"text + scoring": the image codes are then precomputed).  Windows of `iters`
calls are event-timed, (a) and (b) alternating; the medians over `repeats`
windows are reported with their spread.  The two ways' hits and sentence
embeddings are compared on the timed inputs.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'ee-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def loop_hits(img, txt, x, own, cand_caps, cand_lens):
    """(a): the reference's one-by-one loop with this library's forward."""
    with torch.no_grad():
        code = img(x)[1]
        hits = torch.zeros(x.shape[0], dtype=torch.int32, device=code.device)
        T = cand_caps.shape[2]
        for b in range(x.shape[0]):
            rnn = torch.cat([own[b:b + 1], txt(cand_caps[b], cand_lens[b], max_len=T)[1]])
            norm = code[b:b + 1].norm(dim=1, keepdim=True) @ rnn.norm(dim=1, keepdim=True).t()
            hits[b] = torch.argmax((code[b:b + 1] @ rnn.t()) / norm.clamp(min=1e-8)) == 0
    return hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--r', type=int, default=100)
    ap.add_argument('--words', type=int, default=18)
    ap.add_argument('--vocab', type=int, default=5450)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rprec_bench needs a HIP device')
    import DAMSM
    from metrics import r_precision_hits
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    B, R, T = a.batch, a.r, a.words
    txt = DAMSM.RNN_ENCODER(a.vocab, nhidden=256).to(dev).eval()
    img = DAMSM.CNN_ENCODER(256).to(dev).eval()
    x = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
    lens = torch.randint(5, T + 1, (B * R,), device=dev)
    caps = torch.randint(1, a.vocab, (B * R, T), device=dev) * (torch.arange(T, device=dev)[None, :] < lens[:, None])
    own = txt(caps[:B], lens[:B], max_len=T)[1]
    cand_caps, cand_lens = caps[B:].reshape(B, R - 1, T), lens[B:].reshape(B, R - 1)
    with torch.no_grad():
        code = img(x)[1]

    def precomputed(_):
        return None, code

    ways = [('a whole', lambda: loop_hits(img, txt, x, own, cand_caps, cand_lens)),
            ('b whole', lambda: r_precision_hits(img, txt, x, own, cand_caps, cand_lens)),
            ('a text + scoring', lambda: loop_hits(precomputed, txt, x, own, cand_caps, cand_lens)),
            ('b text + scoring', lambda: r_precision_hits(precomputed, txt, x, own, cand_caps, cand_lens))]
    outs = [f() for _, f in ways]   # warm-up: code objects, conv plans, the token table
    outs = [f() for _, f in ways]
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
    med = []
    lines = ['B=%d R=%d T=%d vocab=%d: %d candidate captions per call; %d windows of %d calls, a/b alternating'
             % (B, R, T, a.vocab, B * (R - 1), a.repeats, a.iters)]
    for (name, _), m in zip(ways, ms):
        m.sort()
        med.append(m[len(m) // 2])
        lines.append('%-18s median %.3f ms per call (min %.3f, max %.3f)' % (name, med[-1], m[0], m[-1]))
    lines.append('ratio a / b: whole %.2f, text + scoring %.2f' % (med[0] / med[1], med[2] / med[3]))
    s_old = txt(caps[B:], lens[B:], max_len=T)[1]
    s_new = txt.encode_sentences(caps[B:], lens[B:])
    lines.append('hits equal: %s (%d of %d); sentence embeddings rel L2 new vs old %.3e'
                 % (all(torch.equal(o, outs[0]) for o in outs), int(outs[0].sum()), B,
                    float((s_new - s_old).norm() / s_old.norm())))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
