"""The configuration of dynamic loss scaling, without a GPU: dqnhip_default_config's four defaults, every refusal of the validator
that dqnhip_grad_arena_bytes shares with dqnhip_create (each message names the field), and capi.Config against the header's size."""
import ctypes as C

import pytest


def _cfg(pkg, **kw):
    lib = pkg.capi.load()
    cfg = pkg.capi.Config()
    lib.dqnhip_default_config(C.byref(cfg), 59)
    cfg.minibatch = 128
    cfg.num_hidden = 2
    cfg.hidden[0], cfg.hidden[1] = 128, 128
    cfg.precision = 1
    cfg.loss_scale_mode = pkg.capi.LOSS_SCALE_DYNAMIC
    for k, v in kw.items():
        setattr(cfg, k, v)
    return lib, cfg


def test_defaults_and_struct_size(pkg):
    lib = pkg.capi.load()
    cfg = pkg.capi.Config()
    lib.dqnhip_default_config(C.byref(cfg), 59)
    assert cfg.struct_size == C.sizeof(pkg.capi.Config)
    assert cfg.loss_scale_mode == pkg.capi.LOSS_SCALE_STATIC == 0
    assert cfg.loss_scale_growth_interval == 2000
    assert cfg.loss_scale_min_mult == 2.0 ** -12
    assert cfg.loss_scale_max_mult == 1.0
    # the new fields sit behind tuning_flags, in the header's order
    names = [n for n, _ in pkg.capi.Config._fields_]
    assert names[names.index("tuning_flags") + 1:] == ["loss_scale_mode", "loss_scale_growth_interval", "loss_scale_min_mult", "loss_scale_max_mult"]
    # a wrong struct_size is still an ABI mismatch
    cfg.struct_size -= 16
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) == 0 and b"struct_size" in lib.dqnhip_last_error()


def test_dynamic_fp16_config_is_accepted(pkg):
    lib, cfg = _cfg(pkg)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0
    lib, cfg = _cfg(pkg, loss_scale_growth_interval=0, loss_scale_min_mult=2.0 ** -20, loss_scale_max_mult=8.0)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0
    # static mode reads none of the other fields (a caller that zeroed the struct behind tuning_flags keeps working)
    lib, cfg = _cfg(pkg, loss_scale_mode=0, loss_scale_growth_interval=-5, loss_scale_min_mult=0.0, loss_scale_max_mult=0.0)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0


@pytest.mark.parametrize("kw,field", [
    (dict(precision=0), b"precision"),
    (dict(dp_world=2), b"dp_world"),
    (dict(loss_scale_min_mult=0.3), b"loss_scale_min_mult"),
    (dict(loss_scale_min_mult=0.0), b"loss_scale_min_mult"),
    (dict(loss_scale_min_mult=-0.5), b"loss_scale_min_mult"),
    (dict(loss_scale_max_mult=3.0), b"loss_scale_max_mult"),
    (dict(loss_scale_max_mult=float("inf")), b"loss_scale_max_mult"),
    (dict(loss_scale_min_mult=2.0, loss_scale_max_mult=1.0), b"loss_scale_min_mult"),      # min > max
    (dict(loss_scale_min_mult=2.0, loss_scale_max_mult=4.0), b"loss_scale_min_mult"),      # 1 below [min, max]
    (dict(loss_scale_min_mult=0.25, loss_scale_max_mult=0.5), b"loss_scale_max_mult"),     # 1 above [min, max]
    (dict(loss_scale_growth_interval=-1), b"loss_scale_growth_interval"),
    (dict(loss_scale_mode=2), b"loss_scale_mode"),
])
def test_refusals_name_the_field(pkg, kw, field):
    lib, cfg = _cfg(pkg, **kw)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) == 0
    msg = lib.dqnhip_last_error()
    assert field in msg, msg
    if "loss_scale_mode" not in kw and field != b"loss_scale_mode":
        assert b"loss_scale" in msg
