"""The host's one BatchNorm statistics path: _runtime.bn_args turns an nn.BatchNorm2d into
the argument record every C call takes, and _autograd.update_running is the one running-statistics tail
of the training path.  CPU tensors only: the record holds addresses and plain numbers, nothing is launched."""
import itertools

import pytest
import torch
import torch.nn as nn

from fastfourierconvolution_amd import _autograd as ag
from fastfourierconvolution_amd import _runtime as rt

C, EPS, COUNT_MULT = 3, 3e-4, 2.5
CASES = list(itertools.product((True, False), (True, False), (True, False), (0.1, None)))


def _bn(training, track, affine, momentum):
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=momentum, affine=affine, track_running_stats=track)
    return bn.train(training)


def _addr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("fold", (False, True))
@pytest.mark.parametrize("training,track,affine,momentum", CASES)
def test_bn_args_record(training, track, affine, momentum, fold):
    bn = _bn(training, track, affine, momentum)
    a = rt.bn_args(bn, C, COUNT_MULT, fold=fold)
    update = training and track
    assert a.C == C
    assert (a.gamma, a.beta) == (_addr(bn.weight), _addr(bn.bias))
    assert (a.gamma is None, a.beta is None) == (not affine, not affine)
    stats = (a.running_mean, a.running_var, a.num_batches_tracked)
    if fold and not update:   # an in-kernel fold gets the running statistics only to update them
        assert stats == (None, None, None)
    else:   # None exactly where the module has no tensor
        assert stats == (_addr(bn.running_mean), _addr(bn.running_var), _addr(bn.num_batches_tracked))
        assert [p is None for p in stats] == [not track] * 3
    assert a.update == int(update) and rt.bn_mode(bn)[1] == update
    assert a.momentum == (-1.0 if momentum is None else momentum)
    assert (a.eps, a.count_mult) == (EPS, COUNT_MULT)
    # the run of nine arguments between the moments and the outputs of ffc_bn_finalize, in its order
    assert a[1:] == (a.gamma, a.beta, *stats, a.update, a.momentum, a.eps, a.count_mult)


@pytest.mark.parametrize("fold", (False, True))
def test_bn_args_refuses_another_channel_count(fold):
    bn = _bn(True, True, True, 0.1)
    with pytest.raises(RuntimeError, match=r"running_mean should contain 4 elements not 3"):
        rt.bn_args(bn, C + 1, 1.0, fold=fold)


@pytest.mark.parametrize("training,track,affine,momentum", CASES)
def test_update_running_tail(monkeypatch, training, track, affine, momentum):
    calls = []
    monkeypatch.setattr(torch.ops.ffc, "bn_update_running", lambda *a: calls.append(a), raising=False)
    bn = _bn(training, track, affine, momentum)
    stats = torch.zeros((C, 3), dtype=torch.float64)
    ag.update_running(bn, stats)
    if not (training and track):
        assert calls == []
        return
    (call,) = calls
    assert call[0] is bn.running_mean and call[1] is bn.running_var and call[2] is bn.num_batches_tracked
    assert call[3] is stats
    assert call[4:] == (-1.0 if momentum is None else momentum, 1.0)
