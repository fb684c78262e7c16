"""ops.packed_weight's registry of persistent packed images, with more than one live model in it.

An entry is a list that starts with a weak reference to its Parameter, so comparing two entries with == compares the live
Parameters element-wise: a lookup of a re-homed parameter's old entry has to go by identity, or it raises ("Boolean value of
Tensor with more than one value is ambiguous", or a shape mismatch) as soon as another live entry stands in front of it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def test_rehoming_a_parameter_behind_other_live_entries():
    from sradsgan_amd import ops
    first = torch.nn.Conv2d(16, 32, 3).to(DEV)          # the same shape as the re-homed one: == would be an ambiguous tensor
    second = torch.nn.Conv2d(32, 16, 3).to(DEV)         # another shape: == would not even broadcast
    moved = torch.nn.Conv2d(16, 32, 3).to(DEV)
    for conv in (first, second, moved):
        ops.packed_weight(conv.weight, 0)
    count = len(ops._registry.entries)
    old = moved.weight._srhip_packed[0]
    assert any(e is old for e in ops._registry.entries)
    with torch.no_grad():
        moved.weight.data = moved.weight.data * 2.0     # new storage under the same Parameter, new values
    packed = ops.packed_weight(moved.weight, 0)
    entries = ops._registry.entries
    new = moved.weight._srhip_packed[0]
    assert new is not old and len(entries) == count
    assert not any(e is old for e in entries) and sum(e is new for e in entries) == 1
    for conv in (first, second):
        assert sum(e is conv.weight._srhip_packed[0] for e in entries) == 1
    assert torch.equal(packed, ops.packed_weight(moved.weight.detach().clone(), 0))      # the image of the values it holds now
