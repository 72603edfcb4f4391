"""MI355X parity of the fused residual add + LayerNorm (include/hyena_block.h) through the C ABI against the reference's
unfused graph (src/models/sequence/simple_lm.py:267-271) evaluated in fp64 on the CPU, and at a full HyenaDNA layer
size (2^20 positions x 256 channels) against the same graph in PyTorch ops on the GPU."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _graph(x0, residual, weight, bias, eps, out_dtype):
    res = x0.to(residual.dtype) + residual if residual is not None else x0.to(weight.dtype)
    return F.layer_norm(res.to(weight.dtype), (x0.shape[-1],), weight, bias, eps).to(out_dtype), res


@pytest.mark.parametrize("shape,dtype,with_res", [((2, 37, 64), torch.float32, True), ((3, 1000, 128), torch.bfloat16, True),
                                                  ((1, 4099, 256), torch.bfloat16, False), ((2, 513, 256), torch.float16, True),
                                                  ((1, 77, 1024), torch.bfloat16, True)])
def test_add_norm_vs_fp64_graph(gpu_lib, shape, dtype, with_res):
    from hyena_dna_amd.block import dropout_add_layer_norm
    g = torch.Generator().manual_seed(sum(shape))
    D = shape[-1]
    x0 = torch.randn(shape, generator=g).to(dtype)
    residual = torch.randn(shape, generator=g) * 2 if with_res else None
    weight, bias = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dout, dres = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g)

    def run(dev, fused, wide):
        t = lambda a: None if a is None else (a.double() if wide else a).to(dev)      # noqa: E731
        xs = t(x0).requires_grad_(True)
        rs = None if residual is None else t(residual).requires_grad_(True)
        ws, bs = t(weight).requires_grad_(True), t(bias).requires_grad_(True)
        if fused:
            out, res = dropout_add_layer_norm(xs, rs, ws, bs, 0.0, 1e-5, prenorm=True, residual_in_fp32=True)
        else:
            out, res = _graph(xs, rs, ws, bs, 1e-5, xs.dtype)
        torch.autograd.backward([out, res], [t(dout).to(out.dtype), t(dres).to(res.dtype)])
        return [out.detach(), res.detach(), xs.grad, None if rs is None else rs.grad, ws.grad, bs.grad]

    got = run("cuda", True, False)
    want = run("cpu", False, True)
    ulp = {torch.float32: 2e-6, torch.bfloat16: 2 ** -7, torch.float16: 2 ** -10}[dtype]
    for n, a, r in zip(["out", "residual", "dx0", "dresidual", "dweight", "dbias"], got, want):
        if r is None:
            assert a is None, n
            continue
        if n in ("out", "dx0"):
            assert a.dtype == dtype
            assert (a.double().cpu() - r).abs().max() <= ulp * r.abs().max() + 1e-6, n
        else:
            assert _rel(a, r) < 5e-6, (n, _rel(a, r))


def test_add_norm_at_layer_size(gpu_lib):
    from hyena_dna_amd.block import dropout_add_layer_norm
    B, L, D = 1, 1 << 20, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn(B, L, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
    residual = (torch.randn(B, L, D, device="cuda", generator=g) * 2).requires_grad_(True)
    ln = torch.nn.LayerNorm(D).cuda()
    with torch.no_grad():
        ln.weight.add_(0.2 * torch.randn(D, device="cuda", generator=g))
    dout = torch.randn(B, L, D, device="cuda", generator=g).bfloat16()
    dres = torch.randn(B, L, D, device="cuda", generator=g)

    def run(fused):
        for t in (x0, residual, ln.weight, ln.bias):
            t.grad = None
        if fused:
            out, res = dropout_add_layer_norm(x0, residual, ln.weight, ln.bias, 0.0, ln.eps, prenorm=True, residual_in_fp32=True)
        else:
            out, res = _graph(x0, residual, ln.weight, ln.bias, ln.eps, x0.dtype)
        torch.autograd.backward([out, res], [dout, dres])
        return [out.detach(), res.detach(), x0.grad.clone(), residual.grad.clone(), ln.weight.grad.clone(), ln.bias.grad.clone()]

    a, b = run(True), run(False)
    a2 = run(True)
    for n, x, y, x2 in zip(["out", "residual", "dx0", "dresidual", "dweight", "dbias"], a, b, a2):
        assert torch.equal(x, x2), n                                    # fixed-order reductions: reproducible
        if n in ("out", "dx0"):
            assert (x.float() - y.float()).abs().max() <= 2 ** -7 * y.float().abs().max() + 1e-6, n
        else:
            assert _rel(x, y) < (2e-4 if n in ("dweight", "dbias") else 5e-6), (n, _rel(x, y))   # 1e6-term fp32 sums


def test_tiny_lm_trains_on_the_gpu(gpu_lib):
    """every fused piece in one training loop under bf16 autocast on the MI355X: a 2-layer stack learns periodic DNA"""
    from tests._tiny_lm import train
    # a warmed-up, lower learning rate than the helper's default: the run is stable (round 5 ran at the helper's 3e-3, at the edge of stability, and had
    # to settle for the median of the tail -- ADVICE r5), so the LAST loss is held to the bound and so is every loss of the tail
    losses = train("cuda", steps=40, d=128, L=2048, B=4, n_layer=2, autocast_dtype=torch.bfloat16, lr=1.5e-3, warmup=8)
    assert all(l == l for l in losses)
    assert losses[-1] < 0.35 * losses[0] and max(losses[-5:]) < 0.45 * losses[0], (losses[0], losses[-5:])


def test_tiny_lm_one_step_gradients_match_the_reference_graph(gpu_lib):
    """one training step of the same stack: every parameter gradient of the fused kernels against the SAME modules evaluated by plain PyTorch ops in
    fp32 on the device (the reference's graph: F.linear / F.layer_norm / torch.fft convolution through oracle.hyena_operator) -- a gradient regression
    that a still-converging loss would hide shows here"""
    import torch.nn.functional as F
    from oracle import hyena_oracle as O
    from tests._tiny_lm import TinyLM
    torch.manual_seed(3)
    d, L, B = 128, 1024, 2
    model = TinyLM(16, d, L, 2).cuda()
    ids = torch.randint(7, 11, (B, L), device="cuda")
    tgt = torch.randint(7, 11, (B, L), device="cuda")
    logits = model(ids)
    F.cross_entropy(logits.float().reshape(-1, 16), tgt.reshape(-1)).backward()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)

    def ref_forward(m, ids):
        h, residual = m.emb(ids), None
        for blk in m.blocks:
            residual = h if residual is None else h + residual
            h = F.layer_norm(residual, (d,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
            h = O.hyena_operator(blk.mixer.state_dict(keep_vars=True), h, l_max=L)
            residual = h + residual
            h = F.layer_norm(residual, (d,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
            h = F.linear(F.gelu(F.linear(h, blk.fc1.weight, blk.fc1.bias), approximate="tanh"), blk.fc2.weight, blk.fc2.bias)
        residual = h + residual
        return F.linear(F.layer_norm(residual, (d,), m.ln_f.weight, m.ln_f.bias, m.ln_f.eps), m.emb.weight)

    F.cross_entropy(ref_forward(model, ids).float().reshape(-1, 16), tgt.reshape(-1)).backward()
    assert len(got) > 30
    for n, p in model.named_parameters():
        if p.grad is None:
            continue
        assert n in got, n
        rel = ((got[n] - p.grad).norm() / p.grad.norm().clamp_min(1e-20)).item()
        assert rel < 2e-3, (n, rel)


def test_graphed_train_step_matches_eager(gpu_lib):
    """lm.GraphedTrainStep: forward + loss + backward + AdamW of the whole model captured into ONE hipGraph and replayed on new
    batches gives the eager step's losses and parameters (same kernels, same order; dropout off so no RNG is involved),
    with eager work interleaved between the replays."""
    from hyena_dna_amd.lm import GraphedTrainStep, HyenaDNALM
    dev = torch.device("cuda", 0)
    L, B, D = 2048, 2, 128
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10)

    def make():
        torch.manual_seed(7)
        m = HyenaDNALM(d_model=D, n_layer=2, d_inner=4 * D, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.0,
                       pad_vocab_size_multiple=8).to(dev)
        return m, torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)

    g = torch.Generator(device=dev).manual_seed(3)
    batches = [torch.randint(7, 11, (B, L), generator=g, device=dev) for _ in range(6)]
    warm = 2

    m_e, o_e = make()
    eager = []
    for ids in batches:         # (the graphed step's warm-up updates are undone before the capture: both runs start from the same state)
        o_e.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m_e.loss(ids, torch.roll(ids, -1, 1))
        loss.backward()
        o_e.step()
        eager.append(float(loss.detach()))

    m_g, o_g = make()
    before = [p.detach().clone() for p in m_g.parameters()]
    step = GraphedTrainStep(m_g, o_g, batches[0], torch.roll(batches[0], -1, 1), warmup=warm)
    # the warm-up's optimizer updates are not training steps: parameters, moments and step counters are back where they were
    assert all(torch.equal(a, b) for a, b in zip(before, m_g.parameters()))
    assert all(float(st["step"]) == 0.0 and not bool(st["exp_avg"].any()) for st in o_g.state.values())
    graphed = []
    for ids in batches:
        graphed.append(float(step(ids, torch.roll(ids, -1, 1))))
        # a few hundred eager launches between two replays: what broke replays under the runtime's default graph
        # "packet capture" mode (hyena_dna_amd/__init__.py) -- gradients must stay finite and the losses on track
        assert all(bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(p).all()) for p in m_g.parameters())
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(eager, graphed)), (eager, graphed)
    for (n, p), q in zip(m_e.named_parameters(), m_g.parameters()):
        assert torch.allclose(p, q, rtol=2e-2, atol=2e-4), n

    with pytest.raises(RuntimeError, match="capturable"):
        GraphedTrainStep(m_g, torch.optim.AdamW(m_g.parameters(), lr=1e-3), batches[0], batches[0])
    # releasing the step gives back what the binding kept for its capture stream
    from hyena_dna_amd import _lib
    n_ws = len(_lib._workspace)
    step.release()
    assert len(_lib._workspace) == n_ws - 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype,p", [((2, 4096, 256), torch.float32, 0.1), ((1, 65536, 256), torch.bfloat16, 0.1), ((3, 1000, 128), torch.float16, 0.5)])
def test_fused_dropout_on_gpu(gpu_lib, shape, dtype, p):
    """dropout inside the add + LayerNorm pass on the gfx950 binary: the mask is Philox4x32-10(seed, index) >= p 2^32 (first 4096 elements
    against the Python restatement of the published generator in tests/test_block_emu.py, the keep rate over the whole tensor), the values
    and every gradient are those of the explicit-mask graph, the backward uses the forward's mask."""
    from hyena_dna_amd.block import AddLayerNormFunc
    from tests.test_block_emu import _philox4x32_10
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    D = shape[-1]
    x0 = (torch.randn(shape, generator=g, device=dev) + 3.0).to(dtype).requires_grad_(True)
    residual = (torch.randn(shape, generator=g, device=dev) * 2).requires_grad_(True)
    weight = (1 + 0.2 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    bias = (0.1 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    seed = torch.tensor([0x0BAD_5EED_1234_5678], dtype=torch.int64, device=dev)
    out, res = AddLayerNormFunc.apply(x0, residual, weight, bias, 1e-5, True, p, seed)
    kept = (res.detach() - residual.detach()) != 0
    sv = int(seed.item())
    k0, k1, thr = sv & 0xFFFFFFFF, (sv >> 32) & 0xFFFFFFFF, int(p * 4294967296.0)
    want = [w >= thr for i4 in range(1024) for w in _philox4x32_10(i4, 0, k0, k1)]
    assert kept.reshape(-1)[:4096].cpu().tolist() == want
    assert abs(kept.float().mean().item() - (1 - p)) < 5e-3
    scale = 1.0 / (1.0 - p)
    x0r, rr = x0.detach().double().requires_grad_(True), residual.detach().double().requires_grad_(True)
    wr, br = weight.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    res_r = x0r * kept * scale + rr
    out_r = F.layer_norm(res_r, (D,), wr, br, 1e-5)
    rel = lambda a, b: ((a.double() - b).norm() / b.norm()).item()        # noqa: E731
    assert rel(res, res_r) < 1e-6 and rel(out, out_r) < (2e-6 if dtype == torch.float32 else 5e-3)
    dout, dres = torch.randn(shape, generator=g, device=dev).to(dtype), torch.randn(shape, generator=g, device=dev)
    gx, gr, gw, gb = torch.autograd.grad([out, res], [x0, residual, weight, bias], [dout, dres])
    hx, hr, hw, hb = torch.autograd.grad([out_r, res_r], [x0r, rr, wr, br], [dout.double(), dres.double()])
    tol = 1e-5 if dtype == torch.float32 else 6e-3
    assert rel(gx, hx) < tol and rel(gr, hr) < 1e-5 and rel(gw, hw) < 1e-4 and rel(gb, hb) < 1e-4
    assert torch.equal(gx != 0, kept & (hx != 0))
    out2, res2 = AddLayerNormFunc.apply(x0, residual, weight, bias, 1e-5, True, p, seed)
    assert torch.equal(out2, out) and torch.equal(res2, res)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,D,V,odt,p", [((2, 4096), 256, 16, torch.bfloat16, 0.1), ((1, 70001), 256, 12, torch.float32, 0.0), ((3, 999), 128, 16, torch.float16, 0.3)])
def test_embedding_inside_the_first_add_norm_pass_on_gpu(gpu_lib, shape, D, V, odt, p):
    """the embedding-fused first pass on the gfx950 binary == F.embedding + the (dropout ->) add -> LayerNorm pass with the same seed: residual'
    bit for bit, out up to its one rounding, the table's gradient == the unfused route's (per-token-class sums in a fixed order)"""
    from hyena_dna_amd.block import AddLayerNormFunc, EmbedAddLayerNormFunc
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(sum(shape) + D)
    ids = torch.randint(0, V, shape, generator=g, device=dev)
    table = torch.randn(V, D, generator=g, device=dev).requires_grad_(True)
    weight = (1 + 0.2 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    bias = (0.1 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    seed = torch.tensor([424242424242], dtype=torch.int64, device=dev)
    args = (p, seed) if p > 0 else ()
    out, res = EmbedAddLayerNormFunc.apply(ids, table, weight, bias, 1e-5, odt, *args)
    out_u, res_u = AddLayerNormFunc.apply(F.embedding(ids, table), None, weight, bias, 1e-5, True, *args)
    assert torch.equal(res, res_u)
    if odt == torch.float16:
        # fp16 output: hipcc folds the last multiply-add and the conversion into v_fma_mixlo_f16 -- ONE rounding of the exact result, where the
        # unfused route rounds to fp32 first: the neighbouring fp16 value in a few elements per million
        ref16 = out_u.to(odt)
        assert ((out.float() - out_u).abs() <= 2.0 ** -11 * out_u.abs() + 1e-7).all() and (out != ref16).float().mean().item() < 1e-3
    else:
        assert torch.equal(out, out_u.to(odt))
    dout, dres = torch.randn(shape + (D,), generator=g, device=dev).to(odt), torch.randn(shape + (D,), generator=g, device=dev)
    gt, gw, gb = torch.autograd.grad([out, res], [table, weight, bias], [dout, dres])
    ht, hw, hb = torch.autograd.grad([out_u, res_u], [table, weight, bias], [dout.float(), dres])
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()      # noqa: E731
    assert rel(gt, ht) < 1e-5 and rel(gw, hw) < 1e-5 and rel(gb, hb) < 1e-5
    gt2, _, _ = torch.autograd.grad(EmbedAddLayerNormFunc.apply(ids, table, weight, bias, 1e-5, odt, *args), [table, weight, bias], [dout, dres])
    assert torch.equal(gt2, gt)                                                                             # deterministic
    # ... and DIRECTLY against the graph it replaces, in float64 (not only against this package's own unfused pass):
    #     F.embedding -> dropout mask -> (no residual yet) -> layer_norm, the mask being Philox4x32-10(seed, element index) >= p 2^32
    from tests.test_block_emu import _philox4x32_10
    kept = torch.ones(shape + (D,), dtype=torch.bool, device=dev)
    if p > 0:
        kept = res.detach() != 0                            # (N(0, 1) table entries: a kept element is never exactly zero)
        sv = int(seed.item())
        k0, k1, thr = sv & 0xFFFFFFFF, (sv >> 32) & 0xFFFFFFFF, int(p * 4294967296.0)
        want = [w_ >= thr for i4 in range(256) for w_ in _philox4x32_10(i4, 0, k0, k1)]
        assert kept.reshape(-1)[:1024].cpu().tolist() == want
        assert abs(kept.float().mean().item() - (1 - p)) < 2e-2
    t64 = table.detach().double().requires_grad_(True)
    w64, b64 = weight.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    res_r = F.embedding(ids, t64) * kept * (1.0 / (1.0 - p))
    out_r = F.layer_norm(res_r, (D,), w64, b64, 1e-5)
    assert rel(res, res_r) < 1e-7 and rel(out, out_r) < (2e-6 if odt == torch.float32 else (5e-3 if odt == torch.bfloat16 else 6e-4))
    ft, fw, fb = torch.autograd.grad([out_r, res_r], [t64, w64, b64], [dout.double(), dres.double()])
    assert rel(gt, ft) < 1e-5 and rel(gw, fw) < 1e-4 and rel(gb, fb) < 1e-4
    # an id outside [0, V) reads no memory: its row comes back as NaN (F.embedding device-asserts there), every other row untouched
    bad = ids.clone()
    bad.view(-1)[5] = V
    bad.view(-1)[11] = -1
    out_b, res_b = EmbedAddLayerNormFunc.apply(bad, table.detach(), weight.detach(), bias.detach(), 1e-5, odt, *args)
    rows = torch.ones(ids.numel(), dtype=torch.bool, device=dev)
    rows[5] = rows[11] = False
    assert torch.isnan(res_b.reshape(-1, D)[~rows]).all() and torch.isnan(out_b.reshape(-1, D)[~rows].float()).all()
    assert torch.equal(res_b.reshape(-1, D)[rows], res.detach().reshape(-1, D)[rows])
    # ... and the backward leaves such a row out of every sum (block_kernels.h, AddNormArgs::V), although residual' holds NaN there: the table's,
    # the weight's and the bias's gradients are finite and are those of the remaining rows (the float64 graph with a zero dout / dres on the two rows)
    gt_b, gw_b, gb_b = torch.autograd.grad(EmbedAddLayerNormFunc.apply(bad, table, weight, bias, 1e-5, odt, *args), [table, weight, bias], [dout, dres])
    assert torch.isfinite(gt_b).all() and torch.isfinite(gw_b).all() and torch.isfinite(gb_b).all()
    live = rows.reshape(shape)[..., None].double()
    res_l = F.embedding(ids, t64) * kept * (1.0 / (1.0 - p))
    out_l = F.layer_norm(res_l, (D,), w64, b64, 1e-5)
    lt, lw, lb = torch.autograd.grad([out_l, res_l], [t64, w64, b64], [dout.double() * live, dres.double() * live])
    assert rel(gt_b, lt) < 1e-5 and rel(gw_b, lw) < 1e-4 and rel(gb_b, lb) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,dt,p", [(1 << 20, 256, torch.bfloat16, 0.0), (261888, 128, torch.bfloat16, 0.0), (70001, 256, torch.float16, 0.1), (999, 512, torch.bfloat16, 0.0)])
def test_add_norm_bwd_column_sums_of_dx0_on_gpu(gpu_lib, rows, D, dt, p):
    """hyena_dropout_add_norm_bwd_colsum (round 6): the column sums of the dx0 the kernel writes -- the bias gradient of out_proj / fc2 -- equal a
    float64 column sum of that tensor to fp32 summation accuracy, reach `_lib.colsum` through the side table, and leave every other output bit-identical"""
    from hyena_dna_amd import _gradsum
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(rows % 1000 + D)
    dout = torch.randn(rows, D, generator=g, device=dev).to(dt)
    dres = torch.randn(rows, D, generator=g, device=dev)
    res_out = torch.randn(rows, D, generator=g, device=dev)
    w = 1.0 + 0.2 * torch.randn(D, generator=g, device=dev)
    mean = res_out.mean(1).contiguous()
    rstd = (1.0 / torch.sqrt(res_out.var(1, unbiased=False) + 1e-5)).contiguous()
    seed = torch.tensor([987654321], dtype=torch.int64, device=dev)
    ref = gpu_lib.add_norm_bwd(dout, dres, res_out, w, mean, rstd, dt, need_dres=True, dropout_p=p, seed=seed, offer_colsum=False)
    _gradsum.reset()
    out = gpu_lib.add_norm_bwd(dout, dres, res_out, w, mean, rstd, dt, need_dres=True, dropout_p=p, seed=seed)
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    h0 = _gradsum.stats()["hits"]
    cs = gpu_lib.colsum(out[0])
    assert _gradsum.stats()["hits"] == h0 + 1
    want = out[0].double().sum(0)
    scale = out[0].double().abs().sum(0)
    assert ((cs.double() - want).abs() <= 2e-6 * scale + 1e-6).all()
    own = gpu_lib.colsum(out[0])                                       # the slot is empty now: the streaming kernel's own pass
    assert _gradsum.stats()["hits"] == h0 + 1 and ((own.double() - want).abs() <= 2e-6 * scale + 1e-6).all()
