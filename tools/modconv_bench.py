#!/usr/bin/env python3
"""A/B of the inference generator's fused modulation + 3x3 conv (csrc/conv_mod.hip)
against the composition eegan_bnmod_fwd + eegan_conv_fwd (EEGAN_CONV modconv=0).

Per generator shape (both convs of the seven SAGB blocks: 14 shapes) at C2 (GF = 32,
N = 16) and C3 (GF = 48, N = 32): the two paths run in the same process in
alternating, warmed windows timed with device events; each path's windows together
fill >= --fill seconds.  Reported: the median window per call, the composition's
run-to-run spread ((max - min) / median over its windows) and the dispatch decision
the rule of DESIGN.md §3 takes from them (fused unless slower than the composition
by more than that spread).  Then Gen.infer in images/s: as the library dispatches
it, fused wherever possible (modconv=2), composition (modconv=0), and the eval-mode
Gen.forward (batch statistics: what sampling ran before Gen.infer).

    python tools/modconv_bench.py [--configs C2,C3] [--fill 0.2] [--out profiles/modconv_mi355x.txt]
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'ee-gan_amd'))

import torch  # noqa: E402

CONFIGS = {'C2': (32, 16), 'C3': (48, 32)}
WINDOWS = 7


def gen_shapes(gf):
    """(name, C, K, S, up2, res) of c1 / c2 of every SAGB block (S: the conv's grid)."""
    chans = [(8, 8), (8, 8), (8, 8), (8, 8), (8, 4), (4, 2), (2, 1)]
    out = []
    for b, ((ci, co), S) in enumerate(zip(chans, (4, 8, 16, 32, 64, 128, 256))):
        up2 = b > 0
        out.append(('b%d.c1' % b, ci * gf, co * gf, S, up2, None))
        out.append(('b%d.c2' % b, co * gf, co * gf, S, False, 'half' if up2 else 'full'))
    return out


def set_knob(v):
    items = [kv for kv in os.environ.get('EEGAN_CONV', '').split(',') if kv and not kv.startswith('modconv=')]
    if v is not None:
        items.append('modconv=%d' % v)
    os.environ['EEGAN_CONV'] = ','.join(items)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def ab(fns, fill):
    """Alternating windows of each callable; per callable the list of seconds per call."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    reps = [max(1, int(fill / WINDOWS / max(window(f, 3), 1e-6)) + 1) for f in fns]
    times = [[] for _ in fns]
    for _ in range(WINDOWS):
        for i, f in enumerate(fns):
            times[i].append(window(f, reps[i]))
    return times


def bench_shapes(gf, N, fill, dev, log):
    from eegan_hip import functional as Fn
    from eegan_hip.nn import Conv2d, SyncBatchNorm2d
    from eegan_hip.tensor import to_nhwc_bf16
    log('%-7s %4s %4s %4s %3s %5s | %10s %10s %8s %7s  %s' % ('shape', 'C', 'K', 'S', 'up2', 'res', 'fused us',
                                                                'comp us', 'spread', 'ratio', 'dispatch'))
    for name, C, K, S, up2, res in gen_shapes(gf):
        g = torch.Generator().manual_seed(1)
        conv, bn = Conv2d(C, K, 3, 1, 1, bias=False).to(dev), SyncBatchNorm2d(C, affine=False).to(dev)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        s = S // 2 if up2 else S
        x = to_nhwc_bf16(torch.randn(N, C, s, s, generator=g).to(dev))
        r = to_nhwc_bf16(torch.randn(N, K, *((S // 2,) * 2 if res == 'half' else (S,) * 2), generator=g).to(dev))
        gam, bet = (0.5 * torch.randn(N, C, generator=g).to(dev) for _ in range(2))
        m, gamma = torch.rand(N, 1, S, S, generator=g).to(dev), torch.full((1,), 0.5, device=dev)
        args = (x, conv.weight, conv, bn, gam, bet, m, up2, r, res == 'half', gamma)
        with torch.no_grad():
            tf, tc = ab([lambda: Fn.ModConvFn.apply(*args, True), lambda: Fn.ModConvFn.apply(*args, False)], fill)
        mf, mc = statistics.median(tf), statistics.median(tc)
        spread = (max(tc) - min(tc)) / mc
        log('%-7s %4d %4d %4d %3d %5s | %10.1f %10.1f %7.1f%% %7.3f  %s' % (
            name, C, K, S, up2, res, mf * 1e6, mc * 1e6, 100 * spread, mf / mc,
            'fused' if mf <= mc * (1 + spread) else 'composition'))


def bench_gen(gf, N, fill, dev, log):
    import models
    G = models.Gen(gf, 100).to(dev).eval()
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('gamma') or 'linear2' in n:
                p.normal_(0, 0.3)
    x, sent, attrs = (torch.randn(N, d, device=dev) for d in (100, 256, 256))

    def infer(knob):
        def run():
            set_knob(knob)
            G.infer(x, sent, attrs)
        return run

    def forward():
        with torch.no_grad():
            G(x, sent, attrs)
    names = ['infer (dispatch rule)', 'infer modconv=2', 'infer modconv=0', 'eval forward (batch stats)']
    times = ab([infer(None), infer(2), infer(0), forward], 4 * fill)
    set_knob(None)
    for nm, t in zip(names, times):
        md = statistics.median(t)
        log('Gen GF=%d N=%d %-28s %9.2f ms  %9.1f img/s  (spread %.1f%%)' % (gf, N, nm, md * 1e3, N / md,
                                                                              100 * (max(t) - min(t)) / md))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--fill', type=float, default=0.2)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'profiles', 'modconv_mi355x.txt'))
    ap.add_argument('--gen-only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('modconv_bench needs the GPU: timings are device events')
    dev = torch.device('cuda:0')
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log('modconv_bench on %s: median of %d alternating windows per path, >= %.2f s per path and shape'
        % (torch.cuda.get_device_name(0), WINDOWS, a.fill))
    for cfg in a.configs.split(','):
        gf, N = CONFIGS[cfg]
        log('\n== %s: GF = %d, N = %d' % (cfg, gf, N))
        if not a.gen_only:
            bench_shapes(gf, N, a.fill, dev, log)
        bench_gen(gf, N, a.fill, dev, log)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
