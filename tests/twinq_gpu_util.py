"""What the GPU tests of the off-policy update launches share (test_gpu_td3_critic.py, test_gpu_td3_actor.py, test_gpu_sac_critic.py):
tensors to and from the device, the reference's twin critic in eager torch in a given dtype — what e32 is measured with — and the bar."""
import numpy as np
import torch

from td3_ref import NAMES
from test_td3_critic_host import _Twin


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _idx(index):
    return None if index is None else _cuda(np.asarray(index, dtype=np.int64))


def _twin_module(c, prefix, dtype):
    D, A, H = c["obs"].shape[1], c["action"].shape[1], c[prefix + "fc1_w"].shape[0]
    m = _Twin(D + A, H)
    with torch.no_grad():
        for n in NAMES:
            getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").copy_(torch.from_numpy(c[prefix + n]))
    return m.to(dtype).cuda()


def _q(m, sa, k):
    f = [getattr(m, f"fc{j}") for j in range(3 * k + 1, 3 * k + 4)]
    return f[2](torch.relu(f[1](torch.relu(f[0](sa)))))


def torch_twinq(c, dtype, y, index=None):
    idx = np.arange(130) if index is None else np.asarray(index)
    m = _twin_module(c, "c_", dtype)
    sa = torch.cat([_cuda(c["obs"][idx], dtype), _cuda(c["action"][idx], dtype)], 1)
    yt = _cuda(np.asarray(y), dtype)[:, None]
    m1, m2 = torch.nn.functional.mse_loss(_q(m, sa, 0), yt), torch.nn.functional.mse_loss(_q(m, sa, 1), yt)
    m.zero_grad()
    (m1 + m2).backward()
    grads = {n: _np(getattr(getattr(m, n[:3]), "weight" if n.endswith("w") else "bias").grad).astype(np.float64) for n in NAMES}
    return grads, np.array([(m1 + m2).item(), m1.item(), m2.item(), yt.mean().item()], dtype=np.float64)


def bar(v64, e32):
    return max(2e-6 * max(1.0, float(np.abs(v64).max())), float(e32))
