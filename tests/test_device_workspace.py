"""CPU: device_survey.Workspace, the per-worker buffer object of the device paths of dpred / Jtvec, on torch.device('cpu') -- views of exactly the
requested size over storage that only grows, names that never alias, constants made once per key.  Needs neither the library nor a GPU."""
import torch

from zephyr_amd.device_survey import Workspace


def span(t):
    'the bytes [first, last) a contiguous tensor occupies'
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def test_view_has_the_requested_shape_and_is_contiguous():
    ws = Workspace(torch.device('cpu'))
    for shape, want in ((12, (12,)), ((3, 5), (3, 5)), ((2, 3, 4), (2, 3, 4)), (1, (1,)), ((7, 1), (7, 1))):
        t = ws.buffer('a', shape)
        assert tuple(t.shape) == want and t.is_contiguous() and t.dtype == torch.complex128 and t.device.type == 'cpu'


def test_storage_only_grows():
    ws = Workspace(torch.device('cpu'))
    first = ws.buffer('a', 100)
    p = first.data_ptr()
    assert ws.buffer('a', 100).data_ptr() == p                    # equal: the same storage
    assert ws.buffer('a', (4, 25)).data_ptr() == p                # equal in elements, another shape
    assert ws.buffer('a', 40).data_ptr() == p                     # smaller
    bigger = ws.buffer('a', 101)                                  # larger: new storage (the old one is still held by `first`, so the address differs)
    assert bigger.data_ptr() != p and bigger.numel() == 101
    # a request that shrinks and then grows back below the high-water mark does not reallocate
    q = bigger.data_ptr()
    assert ws.buffer('a', (2, 3)).data_ptr() == q
    assert ws.buffer('a', 101).data_ptr() == q
    assert ws.buffer('a', (10, 10)).data_ptr() == q


def test_what_a_view_holds_survives_a_smaller_request():
    ws = Workspace(torch.device('cpu'))
    a = ws.buffer('a', 8)
    a[:] = torch.arange(8, dtype=torch.float64)
    b = ws.buffer('a', (2, 2))
    assert b.flatten().tolist() == [0, 1, 2, 3]                   # the same memory, its first elements
    b.zero_()
    assert a.tolist() == [0, 0, 0, 0, 4, 5, 6, 7]                 # and a write through the smaller view stops at its end


def test_two_names_never_alias():
    ws = Workspace(torch.device('cpu'))
    views = {name: ws.buffer(name, n) for name, n in (('U', 64), ('R', 64), ('P', 9), ('unit', 9), ('out', (3, 4)))}
    views['U2'] = ws.buffer('U', 16)                              # (a second view of one name does alias it: that is the point)
    assert views['U2'].data_ptr() == views['U'].data_ptr()
    names = ['U', 'R', 'P', 'unit', 'out']
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (a0, a1), (b0, b1) = span(views[a]), span(views[b])
            assert a1 <= b0 or b1 <= a0, (a, b)
    for k, name in enumerate(names):                              # and written through, each keeps its own values
        views[name].fill_(complex(k + 1, -k))
    for k, name in enumerate(names):
        assert bool((views[name] == complex(k + 1, -k)).all())
    # growing one name leaves the others where they are
    before = {name: views[name].data_ptr() for name in names if name != 'P'}
    ws.buffer('P', 1000)
    assert {name: ws.buffer(name, views[name].shape).data_ptr() for name in before} == before


def test_workspaces_share_nothing():
    w1, w2 = Workspace(torch.device('cpu')), Workspace(torch.device('cpu'))
    a, b = w1.buffer('U', 32), w2.buffer('U', 32)
    assert span(a)[1] <= span(b)[0] or span(b)[1] <= span(a)[0]
    assert w1.cached('k', lambda: 1) == 1 and w2.cached('k', lambda: 2) == 2
    assert w1.G is None and w2.G is None


def test_cached_calls_make_once_per_key():
    ws = Workspace(torch.device('cpu'))
    calls = []

    def make(tag):
        def f():
            calls.append(tag)
            return object()
        return f
    a = ws.cached(('csr', None), make('a'))
    assert ws.cached(('csr', None), make('a again')) is a
    b = ws.cached(('csr', (2, 2)), make('b'))
    c = ws.cached(('plan', None), make('c'))
    assert ws.cached(('csr', (2, 2)), make('b again')) is b and ws.cached(('plan', None), make('c again')) is c
    assert calls == ['a', 'b', 'c'] and len({id(a), id(b), id(c)}) == 3
    # a value that is None or False is a value: it is not made again
    assert ws.cached('none', lambda: calls.append('none')) is None and ws.cached('none', lambda: calls.append('none again')) is None
    assert calls == ['a', 'b', 'c', 'none']


def test_cached_keeps_the_object_whose_id_is_the_key_alive():
    import gc
    import weakref

    class Model(object):
        pass
    ws = Workspace(torch.device('cpu'))
    m = Model()
    ref = weakref.ref(m)
    assert ws.cached(('inv_c3', id(m)), lambda: 'inverse', keep=m) == 'inverse'
    del m
    gc.collect()
    assert ref() is not None                                      # (while it lives, no other object can take its id and be served its entry)
    del ws
    gc.collect()
    assert ref() is None
