"""Inference generator: running-statistics modulation fused into the 3x3 conv
(csrc/conv_mod.hip, Fn.ModConvFn, SAGB_Block.infer, Gen.infer, SampleGenerator
running_stats) against float64 restatements of the reference in eval mode
(models.py:69-86,108-126; sync_batchnorm/batchnorm.py:48-53)."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import rel_l2, conv_knob
from oracle.seeding import seeded_state

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _bf(t):
    return t.to(torch.bfloat16).double()


def _nhwc_nan_padded(x, dev):
    """NHWC bf16 activation with 8 padding channels per pixel, all NaN bits."""
    from eegan_hip import tensor as T
    N, C, H, W = x.shape
    t = T.empty_nhwc(N, C, H, W, dev, ld=T.ld_for(C) + 8)
    torch.empty(0, dtype=torch.uint8, device=dev).set_(t.untyped_storage()).fill_(255)
    t.copy_(x.to(dev).to(torch.bfloat16))
    return t


def _modulate64(x, rm, rv, gam, bet, m):
    """relu((gam*m + 1) * BN_eval(x) + bet*m) in float64."""
    xh = F.batch_norm(x, rm.double(), rv.double(), training=False, eps=EPS)
    g, b = gam.double()[:, :, None, None], bet.double()[:, :, None, None]
    return torch.relu((g * m.double() + 1) * xh + b * m.double())


def _layer(C, K, seed, dev):
    """A 3x3 conv and an affine-free norm with non-trivial running buffers."""
    from eegan_hip.nn import Conv2d, SyncBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    conv, bn = Conv2d(C, K, 3, 1, 1, bias=False), SyncBatchNorm2d(C, affine=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(K, C, 3, 3, generator=g) / (3.0 * C ** 0.5))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    return conv.to(dev).eval(), bn.to(dev).eval(), g


# (N, C, Cout, H, W, up2, res): the smallest shape reaching each hazard (H, W = the conv's grid)
KERNEL_CASES = [
    (2, 32, 32, 4, 4, 0, None),        # all-border tile, Cout < 64
    (3, 24, 64, 8, 8, 1, None),        # ragged single slice, up2
    (2, 96, 96, 12, 40, 0, 'full'),    # 3 slices, partial channel tile, crosses the 32-wide and 8-high tile edges
    (2, 48, 48, 10, 34, 1, 'half'),    # ragged second slice, res_up2, 2-pixel tile overhang
    (1, 256, 64, 16, 32, 1, None),     # 8 slices, exact tiles
]


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'N%d_C%d_K%d_%dx%d_up%d_%s' % c)
def test_modconv_kernel_vs_fp64(gpu, case):
    """The fused launch against fp64 (rel_l2 < 1e-2, the bound of bf16-output convs), and no worse
    than 1.5x the error of the bnmod_fwd + conv_fwd composition on the same inputs (a different K
    order and 1-ulp flips of z from the folded fp32 coefficients); finite; bit-reproducible.
    MI355X figures per case: profiles/modconv_mi355x.txt."""
    from eegan_hip import functional as Fn
    N, C, K, H, W, up2, res = case
    conv, bn, g = _layer(C, K, 7 + C + H, gpu)
    h, w = (H // 2, W // 2) if up2 else (H, W)
    x = 2 * torch.randn(N, C, h, w, generator=g) + 0.5
    gam, bet = 0.5 * torch.randn(N, C, generator=g), 0.5 * torch.randn(N, C, generator=g)
    m = torch.rand(N, 1, H, W, generator=g)
    r = None if res is None else torch.randn(N, K, *((H // 2, W // 2) if res == 'half' else (H, W)), generator=g)
    gamma = torch.tensor([0.7])
    # float64 reference from the bf16-rounded operands
    xs = _bf(x)
    if up2:
        xs = F.interpolate(xs, scale_factor=2, mode='nearest')
    z = _bf(_modulate64(xs, bn.running_mean.cpu(), bn.running_var.cpu(), gam, bet, m))
    ref = F.conv2d(z, _bf(conv.weight.detach().cpu()), padding=1)
    if r is not None:
        rr = _bf(r)
        ref = (F.interpolate(rr, scale_factor=2, mode='nearest') if res == 'half' else rr) + 0.7 * ref
    xg = _nhwc_nan_padded(x, gpu)
    rg = None if r is None else _nhwc_nan_padded(r, gpu)
    args = (xg, conv.weight, conv, bn, gam.to(gpu), bet.to(gpu), m.to(gpu), bool(up2), rg, res == 'half',
            gamma.to(gpu) if r is not None else None)
    with torch.no_grad():
        y1 = Fn.ModConvFn.apply(*args, True)
        y2 = Fn.ModConvFn.apply(*args, True)
        yc = Fn.ModConvFn.apply(*args, False)
    assert y1.shape == (N, K, H, W) and torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y2)
    e, ec = rel_l2(y1.float(), ref), rel_l2(yc.float(), ref)
    print('MODCONV %s: fused rel_l2 %.3e  composition %.3e' % (case, e, ec))
    assert e < 1e-2, e
    assert e <= 1.5 * ec, (e, ec)


def test_modconv_rejects_what_it_cannot_run(gpu):
    """C % 8 != 0 and non-3x3 geometries are errors of the entry point (the caller composes), and
    the Function refuses to be recorded by autograd."""
    from eegan_hip import functional as Fn
    from eegan_hip._lib import HipError
    conv, bn, g = _layer(12, 16, 3, gpu)
    x = torch.randn(1, 12, 4, 4).to(gpu)
    args = (x, conv.weight, conv, bn, torch.zeros(1, 12, device=gpu), torch.zeros(1, 12, device=gpu),
            torch.ones(1, 1, 4, 4, device=gpu), False, None, False, None)
    with torch.no_grad():
        with pytest.raises(HipError, match='multiple of 8'):
            Fn.ModConvFn.apply(*args, True)
        assert torch.isfinite(Fn.ModConvFn.apply(*args, None).float()).all()   # the composition
    with pytest.raises(RuntimeError, match='inference only'):
        Fn.ModConvFn.apply(*args, None)


@pytest.mark.parametrize('cin,cout,up2', [(64, 32, True), (32, 32, False)])
def test_sagb_block_infer_vs_fp64(gpu, cin, cout, up2):
    """SAGB_Block.infer (fused, and as the library dispatches it) against models.py:108-126 in eval
    mode restated in float64; the running buffers are not written."""
    import models
    blk = models.SAGB_Block(cin, cout, pred_mask=False)
    blk.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in blk.state_dict().items()], 11))
    blk = blk.to(gpu).eval()
    g = torch.Generator().manual_seed(cin + 1)
    N, S = 2, 8
    feat = torch.randn(N, cin, *((S // 2, S // 2) if up2 else (S, S)), generator=g)
    m = torch.rand(N, 1, S, S, generator=g)
    gb = [(0.5 * torch.randn(N, c, generator=g), 0.5 * torch.randn(N, c, generator=g)) for c in (cin, cout)]
    sd = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
    x = _bf(feat)
    x = F.interpolate(x, scale_factor=2, mode='nearest') if up2 else x
    sc = F.conv2d(x, sd['c_sc.weight'].double(), sd['c_sc.bias'].double()) if blk.learnable_sc else x
    h = x
    for i, cv in ((1, 'c1'), (2, 'c2')):
        h = _modulate64(h, sd['affine%d.norm2d.running_mean' % i], sd['affine%d.norm2d.running_var' % i], *gb[i - 1], m)
        h = F.conv2d(h, sd[cv + '.weight'].double(), padding=1)
    ref = sc + sd['gamma'].double() * h
    gbg = [(a.to(gpu), b.to(gpu)) for a, b in gb]
    for fused in (True, None):
        out, msk = blk.infer(feat.to(gpu), [None, None], m.to(gpu), up2=up2, gb=gbg, fused=fused)
        e = rel_l2(out.float(), ref)
        print('SAGB infer (%d, %d, up2=%s, fused=%s): rel_l2 %.3e' % (cin, cout, up2, fused, e))
        assert msk is None and out.shape == ref.shape and e < 2e-2, e
    for k, v in blk.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k


def test_gen_infer_is_batch_independent_and_stateless(gpu, monkeypatch):
    import models
    G = models.Gen(8, 100)
    G.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in G.state_dict().items()], 21))
    G = G.to(gpu)
    g = torch.Generator().manual_seed(2)
    x, sent, attrs = (torch.randn(3, d, generator=g).to(gpu) for d in (100, 256, 256))
    with pytest.raises(AssertionError):
        G.infer(x, sent, attrs)            # train mode
    G.eval()
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    conv_knob(monkeypatch, 'modconv', 2)   # the fused kernel at every shape it can run
    full = G.infer(x, sent, attrs)
    assert [tuple(o.shape) for o in full] == [(3, 3, s, s) for s in (64, 128, 256)]
    for i in range(3):
        one = G.infer(x[i:i + 1], sent[i:i + 1], attrs[i:i + 1])
        for o, f in zip(one, full):
            assert rel_l2(f[i:i + 1].float(), o.float()) < 1e-2
    conv_knob(monkeypatch, 'modconv', 0)   # the composition everywhere
    for c, f in zip(G.infer(x, sent, attrs), full):
        e = rel_l2(f.float(), c.float())
        print('Gen.infer fused vs composition: rel_l2 %.3e' % e)
        assert torch.isfinite(f.float()).all() and e < 1e-2
    for k, v in G.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # for the record: forward() under eval() normalises its affine_ssa layers with the batch's statistics
    with torch.no_grad():
        fwd, fwd0 = G(x, sent, attrs), G(x[:1], sent[:1], attrs[:1])
    print('Gen.forward (eval) batch of 3 vs alone, rel_l2 per scale: %s'
          % ['%.3e' % rel_l2(f[:1].float(), o.float()) for f, o in zip(fwd, fwd0)])


def _text_only_dataset(root, n_img=8, cpi=10, words=60, seed=5):
    """The test split of a TextOnlyDataset in the reference's layout, as tests/test_gpu_fid.py builds it."""
    rs = np.random.RandomState(seed)
    for d in ('test', 'attributes'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    caps = [[int(t) for t in rs.randint(1, words, size=int(rs.randint(3, 25)))] for _ in range(n_img * cpi)]
    ixtoword = {i: 'w%d' % i for i in range(words)}
    attrs = [[[int(t) for t in rs.randint(1, words, size=int(rs.randint(1, 8)))] for _ in range(int(rs.randint(1, 5)))]
             for _ in range(n_img * cpi)]
    for path, obj in (('captions.pickle', [caps, caps, ixtoword, {v: k for k, v in ixtoword.items()}]),
                      ('attributes/EE-GAN.pickle', [attrs, attrs]),
                      ('test/filenames.pickle', ['t%d' % i for i in range(n_img)]),
                      ('test/class_info.pickle', [1 + i % 3 for i in range(n_img)])):
        with open(os.path.join(root, path), 'wb') as f:
            pickle.dump(obj, f, protocol=2)
    return words


def test_sampler_running_stats(gpu, tmp_path):
    import models
    import DAMSM
    from datasets import TextOnlyDataset
    from metrics.FID.inception import InceptionV3
    from metrics.FID.sampling import SampleGenerator
    words = _text_only_dataset(str(tmp_path))
    nets = [models.Gen(8, 100), models.ATTR_Enhance(), DAMSM.RNN_ENCODER(words, nhidden=256),
            InceptionV3(None, [3])]
    for i, m in enumerate(nets):
        m.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 40 + i))
        m.to(gpu)
    G, A, T, inc = nets
    before = {k: v.detach().clone() for k, v in G.state_dict().items()}
    sampler = SampleGenerator(G, A, T, TextOnlyDataset(str(tmp_path), 'test'), batch_size=4, device=gpu,
                              running_stats=True)
    mu, sigma = sampler.statistics(inc, sampling_nums=8)
    assert mu.shape == (2048,) and sigma.shape == (2048, 2048)
    assert np.isfinite(mu).all() and np.isfinite(sigma).all()
    assert all(torch.equal(v, before[k]) for k, v in G.state_dict().items())
