"""RNN_ENCODER's construction under cfg.RNN_TYPE: a GRU encoder carries torch.nn.GRU's
state_dict keys (a reference GRU checkpoint loads), the LSTM's keys are what they were."""
import pytest
import torch

from _util import spec


def _keys(mod, prefix=''):
    return [(prefix + k, tuple(v.shape)) for k, v in mod.state_dict().items()]


@pytest.mark.parametrize('rnn_type', ['GRU', 'LSTM'])
def test_rnn_type_construction(rnn_type):
    import DAMSM
    from miscc.config import cfg
    old, cfg.RNN_TYPE = cfg.RNN_TYPE, rnn_type
    try:
        enc = DAMSM.RNN_ENCODER(50, nhidden=256)
        assert enc.rnn_type == rnn_type
        hidden = enc.init_hidden(3)
        if rnn_type == 'LSTM':
            assert _keys(enc) == spec('rnn')
            assert len(hidden) == 2 and all(h.shape == (2, 3, 128) for h in hidden)
        else:
            ref = torch.nn.GRU(300, 128, 1, batch_first=True, bidirectional=True)
            assert _keys(enc) == [('encoder.weight', (50, 300))] + _keys(ref, 'rnn.')
            assert torch.is_tensor(hidden) and hidden.shape == (2, 3, 128) and not hidden.any()
            with pytest.raises(NotImplementedError, match='128'):
                DAMSM.RNN_ENCODER(50, nhidden=128)
            with pytest.raises(NotImplementedError):
                DAMSM.RNN_ENCODER(50, nhidden=256, nlayers=2)
            with pytest.raises(NotImplementedError):
                DAMSM.RNN_ENCODER(50, nhidden=256, bidirectional=False)
    finally:
        cfg.RNN_TYPE = old
