"""The fp64 side of the output-refit tests (tests/test_output_fit_host.py, tests/test_gpu_output_fit.py,
tests/golden/make_golden_output_grad.py, tools/output_fit_error.py): the torch composition ``matmul(wt, seq) + bt`` ->
``fit._heads_torch`` -> the restated negative-binomial formula in fp64 under autograd, and the composed a-priori bounds
of DESIGN section 4 "Output refit" with their magnitudes taken from that evaluation.

Parameter order everywhere: ``(wt, bt, w_mu, b_mu, w_sigma, b_sigma)``, the argument order of ``fit.output_nll``."""
import torch

U = 2.0 ** -24
NAMES = ("forecast_time_proj.weight", "forecast_time_proj.bias", "mu_head.weight", "mu_head.bias",
         "sigma_head.weight", "sigma_head.bias")


C = 8                                                           # batch rows of a chunk (TPB_CHUNK)
BS = [1, 2, 3, C - 1, C, C + 1, 2 * C + 3]
LS = [1, 7, 28, 31, 32, 33, 65, 336]
SS = [1, 2, 7, 15, 16, 17, 33, 96, 97]
DS = [4, 8, 24, 64, 96, 128, 136, 512]
# every B, L, S and D appears, rotated against each other; B L D <= 2^20 in every case
GRID = [(BS[i % 7], LS[i % 8], SS[i % 9], DS[(3 * i + i // 8) % 8]) for i in range(36)]
FORMS = {"k_timeproj_bwd_mfma"}                                 # the forms csrc/timeproj_bwd.hip defines


def loss64(fit, seq, p64, tail, hist, y, valid, late, floor, min_sigma):
    """``(loss, rate, dispersion, hidden)`` in fp64 (dispersion >= min_sigma + softplus: away from the band where
    autograd of the formula is no oracle)."""
    wt, bt = p64[:2]
    hidden = torch.matmul(wt, seq.double()) + bt.view(1, -1, 1)
    rate, disp, _ = fit._heads_torch(hidden, *p64[2:], tail.double(), hist, None if late is None else late.double(),
                                     None if floor is None else floor.double(), min_sigma)
    yy = y.double()
    l1 = torch.log1p(disp * rate)
    ll = (torch.lgamma(yy + 1 / disp) - torch.lgamma(1 / disp) - torch.lgamma(yy + 1) - l1 / disp
          + yy * (torch.log(disp) + torch.log(rate) - l1))
    return -(ll * valid).sum() / valid.sum(), rate, disp, hidden


def grads64(fit, seq, params, tail, hist, y, valid, late, floor, min_sigma):
    """The six fp64 gradients of ``loss64`` at the fp32 ``params``."""
    p64 = [p.detach().double().requires_grad_() for p in params]
    return torch.autograd.grad(loss64(fit, seq, p64, tail, hist, y, valid, late, floor, min_sigma)[0], p64)


def grads_and_bounds(fit, seq, params, tail, hist, y, valid, late, floor, min_sigma):
    """``(loss, gradients, bounds)`` in fp64, in the parameter order above.  With R = B S rows, G the loss' gradient in
    the two pre-activations and E = 64 (D + 8 + L + 8) the forward's pre-activation roundings (D + 8 in the heads,
    L + 8 in the time projection) times the bound 1 + y <= 64 on G's logarithmic derivative in a pre-activation:
      heads            (R + 2 + E) 2^-24 sum_r |G[r, n] hidden[r, d]|            (bias: without hidden)
      time projection  (B D + 2 + 2 N + 2 + E) 2^-24 sum_{b, d} (|G_mu| |W_mu| + |G_sg| |W_sg|)[b, s, d] |seq[b, l, d]|
    (the kernel's own summation, k_headfit_dhidden's, the forward's roundings)."""
    p64 = [p.detach().double().requires_grad_() for p in params]
    loss, rate, disp, hidden = loss64(fit, seq, p64, tail, hist, y, valid, late, floor, min_sigma)
    Gm, Gs = torch.autograd.grad(loss, [rate, disp], retain_graph=True)
    want = torch.autograd.grad(loss, p64)
    B, S, D = hidden.shape
    L, N, R = seq.shape[1], p64[2].shape[0], B * S
    low = min_sigma if floor is None else floor.double().reshape(1, 1, -1)
    Gm_pre = (Gm * (1 - torch.exp(-(rate - 1e-6)))).detach().reshape(R, N).abs()     # softplus' = 1 - exp(-softplus)
    Gs_pre = (Gs * (1 - torch.exp(-(disp - 1e-6 - low)))).detach().reshape(R, N).abs()
    Habs = hidden.detach().reshape(R, D).abs()
    E = 64 * (D + 8 + L + 8)
    Kh, Kt = (R + 2 + E) * U, (B * D + 2 + 2 * N + 2 + E) * U
    dH = (Gm_pre @ p64[2].detach().abs() + Gs_pre @ p64[4].detach().abs()).reshape(B, S, D)
    bounds = [Kt * torch.einsum("bsd,bld->sl", dH, seq.double().abs()), Kt * dH.sum((0, 2)),
              Kh * Gm_pre.T @ Habs, Kh * Gm_pre.sum(0), Kh * Gs_pre.T @ Habs, Kh * Gs_pre.sum(0)]
    return loss.detach(), [w.detach() for w in want], bounds


def fraction(got, want, bounds):
    """The largest ``|got - want| / bound`` over the six tensors."""
    return max(float(((a.detach().double().cpu() - b.cpu()).abs() / (bd.cpu() + 1e-300)).max())
               for a, b, bd in zip(got, want, bounds))
