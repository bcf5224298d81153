"""float64 restatement of the reference's edge-aware smoothness(x, y) (Losses/loss_factory.py:183-220), as include/madnet_hip.h states it for
mh_smoothness_loss; shared by tests/test_smoothness_loss.py and tests/test_smoothness_step.py.  TEST INFRASTRUCTURE."""
import torch
import torch.nn.functional as F

KX = [[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]
KY = [[1.0, 2.0, -1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]]          # the -1 top right is the reference's literal (:198)


def stencils(m):
    """m [B,H,W] -> (Kx * m, Ky * m): TF's conv2d = cross-correlation, SAME zero padding, stride 1 (what F.conv2d computes with padding 1)"""
    k = torch.tensor([KX, KY], dtype=m.dtype).view(2, 1, 3, 3)
    o = F.conv2d(m.unsqueeze(1), k, padding=1)
    return o[:, 0], o[:, 1]


def smoothness(disp, image):
    """disp [B,H,W], image [B,H,W,C] (0..255), one dtype, differentiable in disp -> S (a 0-d tensor)"""
    gx, gy = stencils(disp / 255.0)
    ix, iy = stencils((image / 255.0).sum(dim=-1))          # the kernel is concatenated over the input channels: a sum over them
    return (gx.abs() * torch.exp(-ix.abs()) + gy.abs() * torch.exp(-iy.abs())).mean()


def restate(disp, image):
    """float64: (S, dS/ddisp [B,H,W], min over pixels of 255 min(|gx|, |gy|)); the gradient is autograd's, sign(0) = 0 like TF's"""
    d = disp.detach().double().clone().requires_grad_(True)
    s = smoothness(d, image.double())
    g, = torch.autograd.grad(s, [d])
    gx, gy = stencils(d.detach())
    return s.detach(), g, min(gx.abs().min().item(), gy.abs().min().item())


def case(B, H, W, C=3, unambiguous=True):
    """seeded: disparities uniform in (0, 160); image = a horizontal ramp 30 .. 200 plus uniform noise of 40 grey levels (the weights are not all ~ 0); the
    first seed of 1000 * seed + B + H + W at which 255 min(|gx|, |gy|) >= 1e-3, so that every sign is decided in any arithmetic (a 1 x 1 map has gx = 0)"""
    for seed in range(1, 40):
        g = torch.Generator().manual_seed(1000 * seed + B + H + W)
        disp = torch.rand((B, H, W), generator=g) * 160.0
        ramp = 30.0 + 170.0 * torch.arange(W, dtype=torch.float32) / max(W - 1, 1)
        image = ramp.view(1, 1, W, 1) + 40.0 * torch.rand((B, H, W, C), generator=g)
        if not unambiguous or H * W == 1 or restate(disp, image)[2] >= 1e-3:
            return disp, image
    raise AssertionError("no unambiguous seed")
