"""Host side of R-precision: the cluster statistic (test.py:339-357) and the
candidate draw (datasets.py:509-529)."""
import numpy as np
import torch

import _pipeline_data as PD


def test_r_precision_mean_std_matches_reference_loop():
    from metrics import r_precision_mean_std
    hits = (np.random.RandomState(2).rand(40) < 0.4).astype(np.float64)
    np.random.seed(11)
    mean, std = r_precision_mean_std(hits.copy(), 40, clusters=4)
    np.random.seed(11)
    ref = hits.copy()
    np.random.shuffle(ref)
    m = [np.average(ref[ix * 10: (ix + 1) * 10 - 1]) for ix in range(4)]   # 9 of every 10: as the reference
    assert mean == np.average(m) and std == np.std(m)
    assert 0.0 < std and mean != np.average(hits)


def test_get_sent_multi_unpair_draws(tmp_path):
    import datasets as DS
    from miscc.config import cfg
    PD.build(str(tmp_path))
    old = (cfg.TEXT.WORDS_NUM, cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TRAIN.USE_ATTR)
    cfg.TEXT.WORDS_NUM, cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TRAIN.USE_ATTR = 18, PD.CAPS_PER_IMAGE, False
    try:
        ds = DS.TextOnlyDataset(str(tmp_path), 'train')
        R, cls = 8, 1
        np.random.seed(5)
        caps, lens = ds.get_sent_multi_unpair(cls, R)
        after = np.random.get_state()
        assert caps.shape == (R - 1, 18) and caps.dtype == torch.int64
        assert lens.shape == (R - 1,) and lens.dtype == torch.int64
        # the reference's draws: an image index, then a caption index (and get_caption's
        # shuffle for a caption longer than WORDS_NUM), per candidate
        np.random.seed(5)
        for k in range(R - 1):
            i = np.random.randint(0, ds.img_sum)
            while ds.class_id[i] == cls:
                i = (i + 1) % ds.img_sum
            cap, n = ds.get_caption(i * ds.embeddings_num + np.random.randint(0, ds.embeddings_num), ds.captions)
            assert ds.class_id[i] != cls
            assert np.array_equal(caps[k].numpy(), cap.reshape(-1)) and int(lens[k]) == n
        ref = np.random.get_state()
        assert after[0] == ref[0] and np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]
    finally:
        cfg.TEXT.WORDS_NUM, cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TRAIN.USE_ATTR = old
