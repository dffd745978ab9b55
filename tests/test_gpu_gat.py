"""GATConv on the GPU: the additive score through the multi-head SDDMM, the layer against a float64 torch restatement (forward and
every gradient), and two training steps of the example model.

Float64 comparisons use the project's margin for SDDMM-sized sums: |got - ref| <= 1e-4 * max|ref| per compared tensor."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, edge_case_csr

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand(shape, device="cuda", generator=g) - 0.5


# ---------------------------------------------------------------------------------------------------------------- 1. score trick

@pytest.mark.parametrize("H", (1, 4))
def test_additive_score_has_torch_bits(pkg, H):
    """MultiHeadSDDMMFunction on q = (el, 1), k = (1, er) is fl(el[row] + er[col]), bit for bit."""
    import gespmm_amd
    from gespmm_amd import graphs

    G = edge_case_csr()
    rp, ci = _dev(G["rowptr"]), _dev(G["colind"])
    colptr, rowind, order = graphs.transpose_csr(rp, ci, G["K"], return_order=True)
    el, er = _rand((G["M"], H), 1) * 8, _rand((G["K"], H), 2) * 8
    q = torch.stack((el, torch.ones_like(el)), dim=-1)
    k = torch.stack((torch.ones_like(er), er), dim=-1)
    got = gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, order, q, k)
    rows = torch.repeat_interleave(torch.arange(G["M"], device="cuda"), torch.diff(rp).long())
    want = el[rows] + er[ci.long()]
    assert got.shape == want.shape == (G["nnz"], H)
    assert int((got.view(torch.int32) != want.view(torch.int32)).sum()) == 0


# -------------------------------------------------------------------------------------------------------------------- 2. GATConv

def _random_graph(n=300, edges=1700, seed=4):
    """Random directed edges plus every self-loop, duplicates dropped, as CSR with sorted columns: about 2 k entries, no empty row."""
    rng = np.random.RandomState(seed)
    r = np.concatenate((rng.randint(0, n, size=edges), np.arange(n)))
    c = np.concatenate((rng.randint(0, n, size=edges), np.arange(n)))
    key = np.unique(r.astype(np.int64) * n + c)
    r, c = (key // n).astype(np.int32), (key % n).astype(np.int32)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rowptr, c, r


def _gat_float64(x, W, att_dst, att_src, bias, rows, cols, n, H, F, concat, slope):
    xw = (x @ W).view(n, H, F)
    el, er = (xw * att_dst).sum(-1), (xw * att_src).sum(-1)
    e = torch.nn.functional.leaky_relu(el[rows] + er[cols], slope)
    top = torch.full((n, H), -float("inf"), dtype=e.dtype, device=e.device).scatter_reduce(0, rows[:, None].expand(-1, H), e.detach(), "amax")
    t = torch.exp(e - top[rows])  # (softmax does not depend on the shift: no gradient through it)
    alpha = t / torch.zeros((n, H), dtype=e.dtype, device=e.device).index_add_(0, rows, t)[rows]
    out = torch.zeros((n, H, F), dtype=e.dtype, device=e.device).index_add_(0, rows, alpha.unsqueeze(-1) * xw[cols])
    out = out.reshape(n, H * F) if concat else out.mean(dim=1)
    return out + bias


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("heads", (1, 4))
def test_gatconv_against_float64(pkg, heads, concat):
    import gespmm_amd
    from gespmm_amd import graphs

    n, n_in, F = 300, 24, 6
    rowptr, colind, rows_h = _random_graph(n)
    assert 1900 <= colind.size <= 2100 and np.diff(rowptr).min() >= 1
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    torch.manual_seed(7 + heads)
    conv = gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2).cuda()
    with torch.no_grad():
        conv.bias.copy_(_rand(conv.bias.shape, 5))  # (zeros by default: give its gradient a forward to agree with)
    assert conv.weight.shape == (n_in, heads * F) and conv.att_dst.shape == conv.att_src.shape == (1, heads, F)
    assert conv.bias.shape == ((heads * F,) if concat else (F,))
    x = (_rand((n, n_in), 6) * 4).requires_grad_(True)
    gout = _rand((n, heads * F if concat else F), 8)
    out = conv(x, rp, ci, colptr, rowind, order)
    out.backward(gout)
    params = [conv.weight, conv.att_dst, conv.att_src, conv.bias]
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    x64 = x.detach().double().requires_grad_(True)
    ref = _gat_float64(x64, *p64, _dev(rows_h).long(), ci.long(), n, heads, F, concat, float(np.float32(0.2)))
    ref.backward(gout.double())
    pairs = [("out", out.detach(), ref.detach()), ("grad_x", x.grad, x64.grad)]
    pairs += [("grad_" + name, p.grad, q.grad) for name, p, q in zip(("weight", "att_dst", "att_src", "bias"), params, p64)]
    for name, got, want in pairs:
        assert got is not None and got.shape == want.shape, name
        err, scale = (got.double() - want).abs().max().item(), want.abs().max().item()
        print("%s: max err %.3e, max |ref| %.3e" % (name, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)


def test_gatconv_rejects_a_rectangular_graph(pkg):
    import gespmm_amd
    from gespmm_amd import graphs

    G = edge_case_csr()
    rp, ci = _dev(G["rowptr"]), _dev(G["colind"])
    colptr, rowind, order = graphs.transpose_csr(rp, ci, G["K"], return_order=True)
    conv = gespmm_amd.GATConv(5, 3, heads=2).cuda()
    with pytest.raises(ValueError):
        conv(_rand((G["M"], 5), 1), rp, ci, colptr, rowind, order)


# ------------------------------------------------------------------------------------------------------------------- 3. training

def test_two_training_steps_on_cora(pkg):
    """The example's two-layer model (8 heads x 8 features, then 1 head) on cora, dropout off: the loss is finite and goes down."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    device = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = ex.load_edges("cora", device)
    g = ex.gat_graph(edge_index, n_v, device)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(device)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(device)  # the example's training set: 20 nodes per class
    torch.manual_seed(0)
    model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0).to(device)
    assert model.conv1.heads == 8 and model.conv1.out_channels == 8 and model.conv2.heads == 1
    opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
    model.train()

    def loss_now():
        return torch.nn.functional.nll_loss(model(x, g).index_select(0, train_idx), y[train_idx])

    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = loss_now()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(loss_now()))  # what the second step did
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[2] < losses[1], losses
