"""advance_epoch (midastouch_amd/engine.py): the one sparse-scoring epoch rule of every engine form and of the shard state, on a
stand-in holder with CPU tensors.  An epoch is never 0 and never reused while the stamps live, so a stale stamp never equals a
current epoch (the GPU side of the restart: test_gpu_pipelined.py)."""
import types

import torch

import midastouch_amd.engine as E
from midastouch_amd.engine import advance_epoch


def _holder(K=8, lists=False):
    h = types.SimpleNamespace(_epoch=0, _stamps=torch.arange(1, K + 1, dtype=torch.int32))
    if lists:
        h._score_list = torch.arange(1, 3 + 2 * K, dtype=torch.int32)  # two lengths, two lists of K rows: non-zero everywhere
    return h


def test_step_one_without_a_prediction_list():
    h = _holder()
    assert [advance_epoch(h) for _ in range(3)] == [1, 2, 3]
    assert h._epoch == 3


def test_step_two_with_a_prediction_list():
    h = _holder(lists=True)
    assert [advance_epoch(h) for _ in range(3)] == [2, 4, 6]  # (the odd values between them tag the listed rows)
    assert h._epoch == 6


def test_several_frames_at_once():
    h = _holder(lists=True)
    assert advance_epoch(h, 5) == 2 and h._epoch == 10  # a run of 5 frames: epochs 2, 4, ..., 10
    assert advance_epoch(h) == 12
    h = _holder()
    assert advance_epoch(h, 5) == 1 and h._epoch == 5
    assert advance_epoch(h) == 6


def test_restart_zeroes_stamps_and_list_lengths():
    h = _holder(lists=True)
    stamps, lst = h._stamps.clone(), h._score_list.clone()
    h._epoch = E.EPOCH_LIMIT - 4
    assert advance_epoch(h) == E.EPOCH_LIMIT - 2  # the largest epoch there is
    assert torch.equal(h._stamps, stamps) and torch.equal(h._score_list, lst)
    assert advance_epoch(h) == 2  # restarted
    assert h._epoch == 2
    assert not h._stamps.any() and not h._score_list[:2].any()
    assert torch.equal(h._score_list[2:], lst[2:])  # the rows of the lists stay: their lengths are zero


def test_restart_before_a_run_would_cross_the_limit():
    h = _holder(lists=True)
    h._epoch = E.EPOCH_LIMIT - 8
    assert advance_epoch(h, 3) == E.EPOCH_LIMIT - 6 and h._epoch == E.EPOCH_LIMIT - 2  # the run's last epoch is the largest
    assert h._stamps.all()
    assert advance_epoch(h, 2) == 2 and h._epoch == 4
    assert not h._stamps.any() and not h._score_list[:2].any()
    h = _holder()
    h._epoch = E.EPOCH_LIMIT - 1
    assert advance_epoch(h) == 1 and not h._stamps.any()


def test_limit_is_read_at_call_time(monkeypatch):
    monkeypatch.setattr(E, "EPOCH_LIMIT", 7)
    h = _holder()
    assert [advance_epoch(h) for _ in range(8)] == [1, 2, 3, 4, 5, 6, 1, 2]
