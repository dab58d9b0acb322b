"""A handle made by plipmi_clone / plipmi_clone_resolution owns its scratch: the linear-probe and similarity buffers of the source
are never the clone's.  (Before the handle was split into a shared model and per-handle state, a clone made after a probe fit
carried its source's scratch pointers: a larger fit on either freed the other's buffer, and destroying both freed it twice.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from plip_amd import _lib, weights as W
from plip_amd.config import get_config
from plip_amd.engine import Engine, _ptr

pytestmark = pytest.mark.gpu


def _fit(eng, x, y, K):
    """plipmi_probe_fit on K one-vs-rest problems (labels 0 .. K-1) from a zero start -> (WB [K, D + 1], losses [K]) on the host"""
    N, D = x.shape
    ones = torch.ones(K, dtype=torch.float32, device=eng.device)
    wb = torch.zeros((K, D + 1), dtype=torch.float32, device=eng.device)
    info = _lib.ProbeInfo()
    with torch.cuda.device(eng.device):
        rc = eng.lib.plipmi_probe_fit(eng._h, _ptr(x), N, D, _ptr(y), K, _ptr(ones), _ptr(ones), 1.0, 50, 1e-4, _ptr(wb), C.byref(info),
                                      eng._stream())
    assert rc in (0, _lib.ERR_NOT_CONVERGED), _lib.last_error()     # (what is compared is the bits, converged or not)
    torch.cuda.synchronize()
    return wb.cpu().numpy(), np.array(info.loss[:K])


def _problem(n, d, seed, device):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((n, d)).astype(np.float32)).to(device)
    y = torch.from_numpy((rs.rand(n) < 0.5).astype(np.int32)).to(device)
    return x, y


def _destroy_handle_only(eng):
    eng.lib.plipmi_destroy(eng._h)
    eng._h = C.c_void_p()


@pytest.mark.parametrize("first_closed", ["source", "clone"])
@pytest.mark.parametrize("derive", ["clone", "at_resolution"])
def test_clone_owns_its_scratch(derive, first_closed):
    cfg = get_config("tiny")
    src = Engine(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=8)
    D = cfg.projection_dim
    x_small, y_small = _problem(64, D, 1, src.device)
    x_big, y_big = _problem(4096, D, 2, src.device)
    wb0, loss0 = _fit(src, x_small, y_small, 2)                       # the source's scratch exists now
    other = src.clone() if derive == "clone" else src.at_resolution(96, 80)
    wb_big, loss_big = _fit(other, x_big, y_big, 2)                   # the clone's scratch grows: allocations of its own
    wb1, loss1 = _fit(src, x_small, y_small, 2)
    assert np.array_equal(wb0, wb1) and np.array_equal(loss0, loss1)
    assert np.isfinite(wb_big).all() and np.isfinite(loss_big).all()
    rs = np.random.RandomState(3)
    keys = torch.from_numpy(rs.standard_normal((4, D)).astype(np.float32)).to(src.device)
    space = torch.from_numpy(rs.standard_normal((300, D)).astype(np.float32)).to(src.device)
    want = torch.topk(keys.double() @ space.double().T, 5, dim=1).indices
    for eng in (src, other):
        assert torch.equal(eng.similarity_topk(keys, space, 5), want)
    wb2, loss2 = _fit(other, x_small, y_small, 2)                     # and the same problem gives the same bits on either handle
    assert np.array_equal(wb0, wb2) and np.array_equal(loss0, loss2)
    torch.cuda.synchronize()
    first, second = (src, other) if first_closed == "source" else (other, src)
    _destroy_handle_only(first)
    wb3, loss3 = _fit(second, x_small, y_small, 2)                    # the survivor's scratch is still its own
    assert np.array_equal(wb0, wb3) and np.array_equal(loss0, loss3)
    assert torch.equal(second.similarity_topk(keys, space, 5), want)
    torch.cuda.synchronize()
    _destroy_handle_only(second)
    src.close()
    torch.cuda.synchronize()
