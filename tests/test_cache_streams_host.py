"""The state machine of `ops.Ready`, the readiness token of every host-side cache entry, on stub streams and events:
no GPU.  `ops._current_stream`, `ops._current_handle` and `ops._capturing` are the places the token asks torch.cuda; all are replaced
here.  The GPU side -- a cache built on one stream and used on another behind a delay -- is tests/test_gpu_cache_streams.py.
"""
import copy
import pickle

import pytest
import torch

from fincflow_amd import glow, ops

CUDA = torch.device("cuda", 0)


class Event:
    def __init__(self, complete=False):
        self.complete, self.queries = complete, 0

    def query(self):
        self.queries += 1
        return self.complete


class Stream:
    def __init__(self, handle, complete=False):
        self.cuda_stream, self.complete = handle, complete
        self.recorded, self.waited = [], []

    def record_event(self):
        self.recorded.append(Event(self.complete))
        return self.recorded[-1]

    def wait_event(self, event):
        self.waited.append(event)


class Tensor:
    device = CUDA

    def __init__(self):
        self.streams = []

    def record_stream(self, stream):
        self.streams.append(stream)


class World:
    """What the token sees of torch.cuda: the current stream and whether it is capturing."""

    def __init__(self, monkeypatch, stream):
        self.stream, self.capturing, self.asked = stream, False, 0
        monkeypatch.setattr(ops, "_current_stream", self._current)
        monkeypatch.setattr(ops, "_current_handle", lambda device: self._current(device).cuda_stream)
        monkeypatch.setattr(ops, "_capturing", lambda: self.capturing)

    def _current(self, device):
        assert device == CUDA
        self.asked += 1
        return self.stream


def test_the_building_stream_never_waits(monkeypatch):
    s1 = Stream(11)
    world = World(monkeypatch, s1)
    token, t = ops.Ready(CUDA), Tensor()
    assert token.stream == 11 and len(s1.recorded) == 1 and token.event is s1.recorded[0] and not token.done
    for _ in range(3):
        token.wait(t)
    assert s1.waited == [] and t.streams == [] and token.event.queries == 0 and not token.done


def test_another_stream_waits_once_per_use_and_marks_every_tensor(monkeypatch):
    s1, s2 = Stream(11), Stream(12)
    world = World(monkeypatch, s1)
    token = ops.Ready(CUDA)
    world.stream = s2
    a, b = Tensor(), Tensor()
    token.wait(a, None, b)                                   # (None: an entry without its optional tensor, Conv1x1's `_b_lead`)
    assert s2.waited == [token.event] and a.streams == [s2] and b.streams == [s2] and token.event.queries == 1
    assert s1.waited == [] and not token.done
    token.wait(a, None, b)                                   # still in flight: the same again, nothing remembered
    assert s2.waited == [token.event] * 2 and a.streams == [s2, s2] and token.event.queries == 2


def test_a_completed_event_is_never_asked_again(monkeypatch):
    s1, s2 = Stream(11), Stream(12)
    world = World(monkeypatch, s1)
    token, t = ops.Ready(CUDA), Tensor()
    world.stream = s2
    token.wait(t)
    assert token.event.queries == 1 and not token.done
    token.event.complete = True
    token.wait(t)
    assert token.done and token.event.queries == 2 and len(s2.waited) == 1 and t.streams == [s2]
    asked = world.asked
    for _ in range(3):
        token.wait(t)
    # `done` sticks: no query, no wait, not even a look at the current stream
    assert token.event.queries == 2 and len(s2.waited) == 1 and t.streams == [s2] and world.asked == asked


def test_a_capture_refuses_an_entry_in_flight_and_takes_a_finished_one(monkeypatch):
    s1, s2 = Stream(11), Stream(12)
    world = World(monkeypatch, s1)
    token, t = ops.Ready(CUDA), Tensor()
    world.stream, world.capturing = s2, True
    with pytest.raises(RuntimeError, match="synchronise") as e:
        token.wait(t)
    assert str(e.value) == ops.CAPTURE_IN_FLIGHT and "before capturing" in ops.CAPTURE_IN_FLIGHT
    assert s2.waited == [] and t.streams == []               # nothing from outside entered the capture
    token.event.complete = True                              # the caller synchronised: the same capture goes through
    token.wait(t)
    assert token.done and s2.waited == [] and t.streams == []


def test_an_entry_built_inside_a_capture_records_no_event(monkeypatch):
    s1, s2 = Stream(11), Stream(12)
    world = World(monkeypatch, s1)
    world.capturing = True
    token, t = ops.Ready(CUDA), Tensor()
    assert token.event is None and s1.recorded == [] and not token.done
    token.wait(t)                                            # the capturing stream itself: stream order
    world.stream, world.capturing = s2, False
    with pytest.raises(RuntimeError, match="inside a stream capture"):
        token.wait(t)


def test_an_entry_on_the_host_is_born_done(monkeypatch):
    world = World(monkeypatch, Stream(11))
    token = ops.Ready(torch.device("cpu"))
    assert token.done and token.event is None
    token.wait(torch.zeros(1))
    assert world.asked == 0


def _layers_with_derived_values():
    torch.manual_seed(0)
    mix, coupling = glow.Conv1x1(4), glow.Coupling((4, 2, 2), width=4)
    x = torch.randn(2, 4, 2, 2)
    ls, tr = torch.zeros(4), torch.zeros(4)
    with torch.no_grad():
        mix.reverse(x)
        mix.mix_logdet(x)
        coupling._scale_shift_cached()
    # (the folds run on the device only: their entries as the device path leaves them)
    mix._m_aff, mix._b_aff, mix._aff_key, mix._aff_ready = torch.eye(4), tr, ops.version_key(ls, tr), ops.Ready(tr.device)
    mix._m_lead, mix._b_lead, mix._lead_key, mix._lead_inv, mix._lead_obj, mix._lead_ready = torch.eye(4), None, (), mix._w_inv, ls, ops.Ready(tr.device)
    return mix, coupling


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_a_copy_of_a_layer_drops_the_tokens_with_the_caches(how):
    mix, coupling = _layers_with_derived_values()
    unit_cache = ops.PackedWeights()
    unit_cache._banks[torch.device("cpu")] = ops._DeviceBank("key", (), torch.zeros(4, 1, 3, 3))
    assert unit_cache._banks[torch.device("cpu")].ready.done
    for layer in (mix, coupling):
        held = [n for n in layer._derived if n in layer.__dict__]
        assert any(n.endswith("_ready") for n in held) and len(held) == len(layer._derived), (type(layer).__name__, held)
        assert all(isinstance(layer.__dict__[n], ops.Ready) for n in held if n.endswith("_ready"))
        twin = copy.deepcopy(layer) if how == "deepcopy" else pickle.loads(pickle.dumps(layer))
        assert not [n for n in layer._derived if n in twin.__dict__]
        assert len(held) == len([n for n in layer._derived if n in layer.__dict__])          # the original keeps its own
        for (n, p), (m, q) in zip(layer.named_parameters(), twin.named_parameters()):
            assert n == m and torch.equal(p, q) and p.data_ptr() != q.data_ptr()
    with torch.no_grad():                                    # and the copy rebuilds from ITS parameters
        twin_mix = copy.deepcopy(mix)
        twin_mix.W.mul_(2.0)
        x = torch.randn(2, 4, 2, 2)
        assert torch.allclose(twin_mix.reverse(x), mix.reverse(x) / 2.0, atol=1e-6)
        assert isinstance(twin_mix._inv_ready, ops.Ready) and twin_mix._inv_ready is not mix._inv_ready
    twin_cache = copy.deepcopy(unit_cache) if how == "deepcopy" else pickle.loads(pickle.dumps(unit_cache))
    assert twin_cache._banks == {} and len(unit_cache._banks) == 1
