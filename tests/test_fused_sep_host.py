"""Host only: the two tuning fields of the fused separator levels (helm_tuning.nd_fused_sep, nd_fused_sep_min) through the environment and through
helm_set_tuning.  (The GPU tests of the path itself: test_gpu_fused_sep.py.)"""
import os


def test_fused_sep_tuning_fields_round_trip(helm_lib, monkeypatch):
    from zephyr_amd import _lib
    for k in list(os.environ):
        if k.startswith('HELM_'):
            monkeypatch.delenv(k)
    _lib.set_tuning(None)
    t = _lib.tuning()
    assert t.nd_fused_sep == 1 and t.nd_fused_sep_min >= 1
    default_min = t.nd_fused_sep_min
    assert [n for n, _ in _lib.Tuning._fields_][-2:] == ['nd_fused_sep', 'nd_fused_sep_min']          # at the end: the layout of the earlier fields stays
    monkeypatch.setenv('HELM_ND_FUSEDSEP', '0')
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '37')
    t = _lib.tuning()
    assert (t.nd_fused_sep, t.nd_fused_sep_min) == (0, 37)
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '-5')                            # clamped like every other field
    assert _lib.tuning().nd_fused_sep_min == 1
    monkeypatch.delenv('HELM_ND_FUSEDSEP')
    monkeypatch.delenv('HELM_ND_FUSEDSEP_MIN')
    t = _lib.tuning()
    assert (t.nd_fused_sep, t.nd_fused_sep_min) == (1, default_min)
    try:
        t.nd_fused_sep = 0; t.nd_fused_sep_min = 4096
        _lib.set_tuning(t)
        monkeypatch.setenv('HELM_ND_FUSEDSEP', '1')                             # a set structure wins over the environment
        u = _lib.tuning()
        assert (u.nd_fused_sep, u.nd_fused_sep_min) == (0, 4096)
        # a zero-initialised structure: the path off, the threshold at its lower limit
        _lib.set_tuning(_lib.Tuning())
        u = _lib.tuning()
        assert (u.nd_fused_sep, u.nd_fused_sep_min) == (0, 1)
    finally:
        _lib.set_tuning(None)
    assert _lib.tuning().nd_fused_sep == 1
