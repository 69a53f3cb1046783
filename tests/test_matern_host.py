"""The Matern kernel family on the host side (no GPU): the covar_module resolver, the parameter layout, the family codes, and the fp64
closed forms of tests/matern_ref.py pinned against the general Matern formula (scipy) and autograd."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref as MR                                            # noqa: E402
from meta_learning_pacoh_amd import _lib as L                      # noqa: E402
from meta_learning_pacoh_amd.engine import ParamLayout            # noqa: E402
from meta_learning_pacoh_amd.modules import apply_initial_values, resolve_covar_module   # noqa: E402


# stand-ins for the gpytorch classes (recognised by class name: gpytorch is not installed)
class Kernel:
    pass


class MaternKernel(Kernel):
    def __init__(self, nu=2.5, raw=(0.0,)):
        self.nu = nu
        self.raw_lengthscale = torch.nn.Parameter(torch.tensor([list(raw)]))


class BareMaternKernel(Kernel):                                   # a MaternKernel without `nu`
    pass


BareMaternKernel.__name__ = 'MaternKernel'


class ScaleKernel(Kernel):
    def __init__(self, base, raw):
        self.base_kernel, self.raw_outputscale = base, torch.nn.Parameter(torch.tensor(raw))


@pytest.mark.parametrize('nu, kind', [(0.5, 'M12'), (1.5, 'M32'), (2.5, 'M52')])
def test_resolver_accepts_matern(nu, kind):
    k, init, learn = resolve_covar_module(MaternKernel(nu, (0.3,)))
    assert k == kind and not learn
    assert init['lengthscale_raw'] == [pytest.approx(0.3)]
    assert abs(math.log1p(math.exp(init['outputscale_raw'])) - 1.0) < 1e-12     # a plain kernel: unit output scale
    # ScaleKernel wrap with an ARD raw-lengthscale vector
    k, init, learn = resolve_covar_module(ScaleKernel(MaternKernel(nu, (0.5, -1.0, 0.25)), 0.75))
    assert k == kind and learn
    assert init['lengthscale_raw'] == [pytest.approx(0.5), pytest.approx(-1.0), pytest.approx(0.25)]
    assert init['outputscale_raw'] == pytest.approx(0.75)
    # the ARD values land in the lengthscale block, one per input dimension
    lay = ParamLayout(3, 'constant', k, with_outputscale=True)
    theta = torch.zeros(lay.D)
    apply_initial_values(theta, lay, init)
    lo, hi = lay.slices['lengthscale_raw']
    assert theta[lo:hi].tolist() == [pytest.approx(0.5), pytest.approx(-1.0), pytest.approx(0.25)]


@pytest.mark.parametrize('bad', [BareMaternKernel(), MaternKernel(nu=3.5), MaternKernel(nu=1.0), ScaleKernel(MaternKernel(nu=0.25), 0.0)])
def test_resolver_refuses_other_matern(bad):
    with pytest.raises(NotImplementedError):
        resolve_covar_module(bad)


@pytest.mark.parametrize('kind, code', [('M12', 3), ('M32', 4), ('M52', 5)])
def test_param_layout_matern(kind, code):
    lay = ParamLayout(3, 'zero', kind, with_outputscale=True)
    assert lay.kernel_code == code and lay.feature_dim == 3
    assert lay.blocks['lengthscale_raw'] == 3                     # ARD, not tied like the cosine period
    assert lay.D == 3 + 1 + 1
    assert (L.KERNEL_MATERN12, L.KERNEL_MATERN32, L.KERNEL_MATERN52) == (3, 4, 5)
    assert L._kf(2, code) == 2 | (code << L.KERNEL_SHIFT)
    assert MR.CODE == {0.5: 3, 1.5: 4, 2.5: 5}


def test_family_codes_in_header():
    """the codes of the C ABI, as the header defines them (code 2 stays unassigned)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'pacoh_gp.h')) as fh:
        text = fh.read()
    for name, code in (('MATERN12', 3), ('MATERN32', 4), ('MATERN52', 5)):
        assert '#define PACOH_KERNEL_%s %d' % (name, code) in text
    assert not any(line.startswith('#define PACOH_KERNEL_') and line.split()[-1] == '2' for line in text.splitlines())


@pytest.mark.parametrize('nu', MR.NUS)
def test_closed_form_matches_general_matern(nu):
    special = pytest.importorskip('scipy.special')
    s = np.concatenate([np.logspace(-6, 1.5, 60), [0.1, 0.5, 1.0, 2.0, 5.0]])
    a = math.sqrt(2 * nu) * s
    general = 2 ** (1 - nu) / special.gamma(nu) * a ** nu * special.kv(nu, a)
    closed = MR.matern_of_s(torch.tensor(s, dtype=torch.float64), nu).numpy()
    np.testing.assert_allclose(closed, general, rtol=1e-12, atol=0)
    assert float(MR.matern_of_s(torch.zeros(1, dtype=torch.float64), nu)) == 1.0


@pytest.mark.parametrize('nu', MR.NUS)
def test_kd_matches_autograd(nu):
    s = torch.tensor(np.concatenate([np.logspace(-8, 1.5, 50), [1e-3, 0.7, 3.0]]), dtype=torch.float64, requires_grad=True)
    k = MR.matern_of_s(s, nu)
    (dk,) = torch.autograd.grad(k.sum(), s)
    kd = MR.kd_of_s(s.detach(), nu)
    ref = -dk / s.detach()
    big = s.detach() > 1e-3                 # (below, autograd's derivative of (1 + a) e^-a cancels: relative error ~1e-16 / s)
    torch.testing.assert_close(kd[big], ref[big], rtol=1e-12, atol=0)
    torch.testing.assert_close(kd, ref, rtol=1e-6, atol=0)
    # s -> 0: the limits (nu = 3/2: 3, nu = 5/2: 5/3) and nu = 1/2's clamp form, 0 at coincident points
    z = MR.kd_of_s(torch.zeros(1, dtype=torch.float64), nu)
    assert float(z) == {0.5: 0.0, 1.5: 3.0, 2.5: 5.0 / 3.0}[nu]
    if nu != 0.5:
        assert float(MR.kd_of_s(torch.tensor([1e-9], dtype=torch.float64), nu)) == pytest.approx(float(z), rel=1e-8)


def test_gradient_through_gram_uses_kd():
    """d K_ij / d u_j = os kd(s) (u_i - u_j) for every family: the convention the device kernels contract with"""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(5, 2, generator=g, dtype=torch.float64)
    ls = torch.tensor([0.7, 1.3], dtype=torch.float64)
    for nu in MR.NUS:
        zz = z.clone().requires_grad_(True)
        K = MR.gram(zz, zz, ls, 1.0, nu)
        (dz,) = torch.autograd.grad(K[0, 1], zz)
        u = z / ls
        s = (u[0] - u[1]).norm()
        want = MR.kd_of_s(s, nu) * (u[0] - u[1]) / ls
        torch.testing.assert_close(dz[1], want, rtol=1e-10, atol=1e-14)
