"""PopTrackPredictor on the device: every g21 fixture replayed bit for bit (the popularity vector after every call and a query of every
node), id widths, and the reference's refusal of float ids in a query."""
import numpy as np
import pytest
import torch

from golden_util import load
from test_tcomem_cpu import POPTRACK, calls_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TORCH = {'int64': torch.int64, 'int32': torch.int32}


def dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dtype).to(DEV)


@pytest.mark.parametrize('name', ['g21_poptrack_' + n for n in POPTRACK])
def test_fixture_replayed_bit_for_bit(name):
    from tgm_amd.nn import PopTrackPredictor

    meta, a = load(name)
    sd = TORCH[meta['stream_dtype']]
    model = None
    for c, (s, d, t) in enumerate(calls_of(meta, a)):
        if model is None:
            model = PopTrackPredictor(dev(s, sd), dev(d, sd), dev(t, sd), meta['num_nodes'], meta['k'], meta['decay'])
        else:
            model.update(dev(s, sd), dev(d, sd), dev(t, sd))
        assert model.popularity.dtype == torch.float32 and model.popularity.device.type == 'cuda'
        assert np.array_equal(model.popularity.cpu().numpy(), a[f'pop{c}'])
        got = model(dev(a['q_src'], sd), dev(a['q_dst'], sd))
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), a[f'q{c}_pred'])
    assert model.k == meta['k'] and model.decay == meta['decay']


def test_float_ids_in_a_query_raise_index_error():
    from tgm_amd.nn import PopTrackPredictor

    model = PopTrackPredictor(dev([0, 1]), dev([2, 3]), dev([1, 2]), num_nodes=4, k=2, decay=0.7)
    assert model(dev([1]), dev([1])).item() == 0.0
    model.update(dev([1]), dev([1]), dev([7], torch.float32))  # the reference's unit test hands a float timestamp over
    assert model(dev([1]), dev([1])).item() == float(np.float32(0.7))
    with pytest.raises(IndexError):
        model(dev([1], torch.float32), dev([1], torch.float32))
    with pytest.raises(IndexError):
        model(dev([1]), dev([1], torch.float64))
