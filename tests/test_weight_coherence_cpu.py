"""What the packed-weight caches of sradsgan_amd.ops lean on, checked without a device.

ops.packed_weight refreshes a cached image when the parameter's `_version` or `data_ptr()` has moved.  Some ways of writing a parameter
move neither: the table below records, for the installed torch, which do.  A torch upgrade that changes a cell fails here, not silently
on the device; tests/test_weight_coherence_gpu.py holds the caches to every row.  The second test keeps the package itself from writing
a parameter in the silent way."""
import ast
import copy
import io
import os

import pytest
import torch
import torch.nn as nn

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sradsgan_amd')


def _fresh():
    torch.manual_seed(0)
    return nn.Conv2d(4, 4, 3)


def _copy_(m):
    with torch.no_grad():
        m.weight.copy_(torch.randn_like(m.weight))


def _init_normal(m):
    nn.init.normal_(m.weight)


def _load_state_dict(m):
    m.load_state_dict({k: torch.randn_like(v) for k, v in m.state_dict().items()})


def _load_state_dict_assign(m):
    m.load_state_dict({k: torch.randn_like(v) for k, v in m.state_dict().items()}, assign=True)


def _optimizer(cls, **kw):
    def run(m):
        opt = cls(m.parameters(), lr=0.1, **kw)
        m.weight.grad = torch.ones_like(m.weight)
        m.bias.grad = torch.ones_like(m.bias)
        opt.step()
    return run


def _data_assign(m):
    m.weight.data = m.weight.data * 2.0


def _vector_to_parameters(m):
    vec = torch.nn.utils.parameters_to_vector(m.parameters())
    torch.nn.utils.vector_to_parameters(vec * 2.0, m.parameters())


def _detach_mul_(m):
    m.weight.detach().mul_(2.0)


def _data_normal_(m):
    m.weight.data.normal_()


def _init_normal_on_data(m):
    nn.init.normal_(m.weight.data, 0.0, 0.02)


def _data_clamp_(m):
    m.weight.data.clamp_(-0.01, 0.01)


def _ema_through_data(m):
    m.weight.data.mul_(0.9).add_(torch.ones_like(m.weight), alpha=0.1)


def _foreach_on_data(m):
    torch._foreach_mul_([m.weight.data], 2.0)


# channel -> (moves _version, moves data_ptr()), on a CPU Parameter.  (False, False) is a silent write: ops.weights_changed is for those.
TABLE = [
    ('no_grad copy_', _copy_, True, False),
    ('nn.init.normal_(p)', _init_normal, True, False),
    ('load_state_dict', _load_state_dict, True, False),
    ('load_state_dict(assign=True)', _load_state_dict_assign, None, True),       # a new Parameter object: its version is not compared
    ('Adam foreach', _optimizer(torch.optim.Adam, foreach=True), True, False),
    ('Adam single', _optimizer(torch.optim.Adam, foreach=False), True, False),
    ('SGD foreach', _optimizer(torch.optim.SGD, foreach=True), True, False),
    ('SGD single', _optimizer(torch.optim.SGD, foreach=False), True, False),
    ('p.data = new', _data_assign, None, True),                                  # the version counter is replaced with the storage
    ('vector_to_parameters', _vector_to_parameters, None, True),                 # assigns p.data a view of the vector
    ('p.detach().mul_', _detach_mul_, True, False),
    ('p.data.normal_', _data_normal_, False, False),
    ('nn.init.normal_(p.data)', _init_normal_on_data, False, False),
    ('p.data.clamp_', _data_clamp_, False, False),
    ('EMA through .data', _ema_through_data, False, False),
    ('_foreach_mul_ on .data', _foreach_on_data, False, False),
]


@pytest.mark.parametrize('name,change,version_moves,ptr_moves', TABLE, ids=[row[0] for row in TABLE])
def test_which_writes_to_a_parameter_torch_reports(name, change, version_moves, ptr_moves):
    m = _fresh()
    before = m.weight.detach().clone()
    version, ptr = m.weight._version, m.weight.data_ptr()
    change(m)
    assert not torch.equal(m.weight.detach(), before), 'the change did nothing'
    assert (m.weight.data_ptr() != ptr) == ptr_moves
    if version_moves is not None:
        assert (m.weight._version != version) == version_moves
    else:
        assert ptr_moves                          # a row that does not pin the version must be seen through the pointer


def test_deepcopy_and_pickle_of_a_parameter_take_plain_attributes_along_or_not():
    """copy.deepcopy of a Parameter drops the attributes of the object; pickling takes its __dict__ along -- which is why the cache
    entries ops keeps there (ops._Slots) have to pickle as empty."""
    p = nn.Parameter(torch.randn(3))
    p._mark = 'x'
    assert not hasattr(copy.deepcopy(p), '_mark')
    buf = io.BytesIO()
    torch.save(p, buf)
    buf.seek(0)
    assert torch.load(buf, weights_only=False)._mark == 'x'


# ---------------------------------------------------------------------------------------------------------------------------------- #

def _is_data(node):
    return isinstance(node, ast.Attribute) and node.attr == 'data'


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
    return '.'.join(reversed(parts))


def silent_writes(source):
    """(line, text) of every in-place write through `.data`: `<x>.data.<name>_(...)`, and `<...>init.<name>_(<x>.data, ...)`."""
    found = []
    for node in ast.walk(ast.parse(source)):
        if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
            continue
        name = node.func.attr
        if not name.endswith('_') or name.endswith('__'):
            continue
        if _is_data(node.func.value):
            found.append((node.lineno, '%s.%s' % (_dotted(node.func.value), name)))
        elif node.args and _is_data(node.args[0]) and _dotted(node.func.value).endswith('init'):
            found.append((node.lineno, '%s.%s(%s)' % (_dotted(node.func.value), name, _dotted(node.args[0]))))
    return found


def test_the_walker_finds_each_form_of_silent_write():
    src = ('m.weight.data.normal_(0, 1)\n'
           'torch.nn.init.normal_(m.weight.data, 0.0, 0.02)\n'
           'init.constant_(m.bias.data, 0.0)\n'
           'ema.data.mul_(d).add_(p.data, alpha=1 - d)\n'
           'with torch.no_grad():\n    m.weight.normal_(0, 1)\n'
           'view.copy_(p.data)\n'
           'x = p.data.clone()\n'
           'p.data = view\n')
    assert [line for line, _ in silent_writes(src)] == [1, 2, 3, 4]


def test_no_function_of_the_package_writes_a_parameter_through_data():
    """dp.ParamArena.__init__ re-homes each parameter (`view.copy_(p.data); p.data = view`): that moves data_ptr() and is no in-place write
    through `.data`, so the walker does not see it and nothing needs an exemption."""
    found = []
    for root, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith('.py'):
                path = os.path.join(root, f)
                with open(path) as fh:
                    found += ['%s:%d %s' % (os.path.relpath(path, PKG), line, what) for line, what in silent_writes(fh.read())]
    assert not found, 'in-place writes through .data leave _version where it was (ops.packed_weight cannot see them):\n' + '\n'.join(found)
