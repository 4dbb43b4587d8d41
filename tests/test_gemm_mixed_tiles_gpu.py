"""Decode GEMM with column tiles of two widths in one launch (gemm.hip gemm_tile_mixed_kernel,
plan kind 8 = [8, stages, 0, narrow width, BM, wide width, sk]).

Each output element's K order does not depend on the tile width or the wave layout (K-tiles of
64, two 32-deep MFMA steps, the same MFMA), so the mixed plan must be bitwise the uniform
128-column tile plan, on the row-major and on the pack_w256 weight, for every epilogue of the
tile kernel. N = 1792 = 8 x (128 + 96) is the smallest N that is also a multiple of 256 (packed
copy): 8 wide tiles over columns [0, 1024) and 8 narrow ones from 1024 on, several of which
straddle a 256-row pack block (1216, 1504, ...)."""
import pytest
import torch

from butterfly_amd import ops
from butterfly_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 1792
KS = (64, 192, 1024)          # one K-tile, fewer tiles than the pipeline prologue, ring wrap
MS = ((64, 64, 2), (37, 64, 2), (16, 16, 1), (1, 16, 1), (37, 32, 1))   # (M, BM, uniform plan's WMW)


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


@pytest.fixture()
def every_shape():
    """Mixed tiles for every decode tile plan whose N splits (mode 2), restored afterwards."""
    prev = torch.ops.bfly.gemm_mixed_tiles_mode(2)
    yield
    torch.ops.bfly.gemm_mixed_tiles_mode(prev)


def _uniform(fn):
    prev = torch.ops.bfly.gemm_mixed_tiles_mode(0)
    try:
        return fn()
    finally:
        torch.ops.bfly.gemm_mixed_tiles_mode(prev)


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _close(a, b, atol, rtol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{bad}/{a.numel()} mismatches, max err {err.max().item():.4g}"


_cache: dict = {}


def _operands(K):
    """x rows (64), the weight, its packed copy and the fp32 product, made once per K."""
    if K not in _cache:
        x, w = _bf(64, K, seed=300 + K), _bf(N, K, scale=0.05, seed=301 + K)
        _cache[K] = (x, w, ops.pack_w256(w), x.float() @ w.float().t())
    return _cache[K]


def _run(x, w, plan, epi, sk, packed=False):
    M = x.shape[0]
    ws = torch.zeros(16384 + sk * M * N + 16, dtype=torch.float32, device=DEV) if sk > 1 else None
    out = torch.empty(M, N // 2 if epi == "silu" else N, dtype=torch.bfloat16, device=DEV)
    torch.ops.bfly.gemm_with_plan(x, w, out, plan, ops.EPILOGUES[epi], ws, None, packed)
    off = torch.ops.bfly.gemm_slab_offset()
    return out, (ws[off:off + sk * M * N].clone() if sk > 1 else None)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,bm,wmw", MS)
def test_mixed_plan_is_bitwise_the_uniform_plan(M, bm, wmw, K):
    """None and SwiGLU epilogues, split-K 1 and 3 (the f32 slabs a deferred consumer would read
    and the reduced output), row-major and packed weight: bitwise the uniform plan, and within
    the project's GEMM tolerance of the fp32 product."""
    x64, w, wp, full = _operands(K)
    x = x64[:M]
    want32 = full[:M]
    for epi in ("none", "silu"):
        for sk in (1, 3):
            if sk > K // 64:
                continue
            base, base_slabs = _run(x, w, [1, 3, 0, wmw, bm, 128, sk], epi, sk)
            for packed in (False, True):
                got, slabs = _run(x, wp if packed else w, [8, 3, 0, 96, bm, 128, sk], epi, sk, packed)
                assert torch.equal(got, base), (epi, sk, packed)
                if sk > 1:
                    assert torch.equal(slabs, base_slabs), (epi, sk, packed)
            if epi == "none":
                _close(base, want32, 2e-2, 2e-2)
            else:
                _close(base, ref.linear(x.cpu(), w.cpu(), None, "silu"), 2e-2, 2e-2)


@pytest.mark.parametrize("M,K", [(64, 192), (37, 2048), (24, 192), (16, 192), (5, 2048), (37, 64)])
def test_mixed_plan_behind_row_split_rmsnorm(every_shape, M, K):
    """SwiGLU behind a row-split RMSNorm (the 1/rms row scale in the GEMM epilogue; K = 2048
    splits K, so the scale lands in the slabs), through ops.linear on both weights."""
    x, w = _bf(M, K, seed=310), _bf(N, K, scale=0.05, seed=311)
    wp = ops.pack_w256(w)
    res = _bf(M, K, seed=312)
    nw = (1.0 + 0.1 * _bf(K, seed=313).float()).to(torch.bfloat16)

    def run(packed):
        xin = ops.rms_norm(x, nw, 1e-5, residual=res.clone(), rows=True)
        return ops.linear(xin, w, epilogue="silu", packed=packed).clone()

    want = _uniform(lambda: run(None))
    # (M <= 4 plans the register-streaming kernel, which takes no row scale: 5 rows stand in
    # for the 1-row case of the explicit-plan test above)
    assert ops.gemm_plan(M, N, K)["kind"] == "mixed", ops.gemm_plan(M, N, K)
    assert torch.ops.bfly.gemm_packed_check(M, N, K, ops.EPILOGUES["silu"]) == 0
    assert torch.equal(run(None), want)
    assert torch.equal(run(wp), want)
    # fp32 product of what the kernel multiplies: bf16 rows (x + res) * g, scaled by 1/rms
    rr = (x.float() + res.float()).to(torch.bfloat16).float().cpu()
    yb = (rr * nw.float().cpu()).to(torch.bfloat16).float()
    prod = (yb @ w.float().cpu().t()) * torch.rsqrt(rr.pow(2).mean(-1, keepdim=True) + 1e-5)
    gate, up = ref.split_gate_up(prod, ref.SILU_INTERLEAVE)
    _close(want, torch.nn.functional.silu(gate) * up, 2e-2, 2e-2)


@pytest.mark.parametrize("M,K", [(64, 192), (37, 64), (16, 192)])
def test_mixed_plan_moe_gate_epilogue(every_shape, M, K):
    """The MoE gate epilogue with 8 local experts of 112 output columns: expert boundaries every
    224 weight rows fall inside wide tiles (224 in [128, 256)) and narrow ones (1344 in
    [1312, 1408))."""
    El, e0, E = 8, 1, 10
    x, w = _bf(M, K, seed=320), _bf(N, K, scale=0.05, seed=321)
    wp = ops.pack_w256(w)
    g = torch.Generator(device="cpu").manual_seed(322)
    gates = torch.rand(M, E, generator=g)
    gates[torch.rand(M, E, generator=g) < 0.3] = 0.0
    gates = gates.to(DEV)
    want = _uniform(lambda: ops.linear_silu_gate(x, w, gates, e0, El))
    assert ops.gemm_plan(M, N, K)["kind"] == "mixed", ops.gemm_plan(M, N, K)
    assert torch.equal(ops.linear_silu_gate(x, w, gates, e0, El), want)
    out = torch.empty_like(want)
    assert torch.ops.bfly.gemm_packed(x, wp, out, 3, None, 0.0, gates, e0, El) > 0
    assert torch.equal(out, want)
    w32 = ref.linear(x.cpu(), w.cpu(), None, "silu")
    ref.moe_gate_scale(w32, gates.cpu(), e0, El)
    _close(want, w32, 2e-2, 2e-2)


@pytest.mark.parametrize("M", [64, 16])
def test_mixed_plan_deferred_slabs(every_shape, M):
    """ops.linear(defer=True) on a shape whose plan splits K: the slabs left for the consumer and
    the materialised result are bitwise the uniform plan's, on both weights."""
    K = 2048
    x, w = _bf(M, K, seed=330), _bf(N, K, scale=0.05, seed=331)
    wp = ops.pack_w256(w)

    def run(packed):
        y = ops.linear(x, w, defer=True, packed=packed)
        assert isinstance(y, ops.Partial)
        slabs = y.slabs.clone()
        return slabs, ops.materialize(y).clone()

    want_slabs, want = _uniform(lambda: run(None))
    p = ops.gemm_plan(M, N, K)
    assert p["kind"] == "mixed" and p["splitk"] > 1, p
    for packed in (None, wp):
        slabs, got = run(packed)
        assert torch.equal(slabs, want_slabs) and torch.equal(got, want)
    _close(want, x.float() @ w.float().t(), 2e-2, 2e-2)


def test_shapes_without_a_width_solution_are_refused():
    """An N that is no multiple of 128 + 96 has no equal split: the dry-run check refuses the
    plan and the launcher raises without launching; other widths have no kernel."""
    mixed = [8, 3, 0, 96, 64, 128, 1]
    for packed in (False, True):
        assert torch.ops.bfly.gemm_plan_check(mixed, 64, N, 192, 0, packed) == 0
    assert torch.ops.bfly.gemm_plan_check(mixed, 64, N + 32, 192, 0, False) < 0
    assert torch.ops.bfly.gemm_plan_check(mixed, 64, N + 32, 192, 2, False) < 0
    assert torch.ops.bfly.gemm_plan_check(mixed, 64, 7 * 224, 192, 0, True) < 0      # packed: N % 256
    assert torch.ops.bfly.gemm_plan_check([8, 3, 0, 112, 64, 128, 1], 64, 240 * 8, 192, 0, False) < 0
    assert torch.ops.bfly.gemm_plan_check([8, 3, 0, 96, 64, 128, 4], 64, N, 192, 0, False) < 0   # 3 K-tiles
    x, w = _bf(64, 192, seed=340), _bf(N + 32, 192, scale=0.05, seed=341)
    out = torch.full((64, N + 32), 7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="plan rejected"):
        torch.ops.bfly.gemm_with_plan(x, w, out, mixed, 0, None)
    assert (out == 7.0).all()
    prev = torch.ops.bfly.gemm_mixed_tiles_mode(2)
    try:
        assert ops.gemm_plan(64, N + 32, 192)["kind"] == "tile"
    finally:
        torch.ops.bfly.gemm_mixed_tiles_mode(prev)


def test_packed_marker_on_a_row_major_weight_runs_exact():
    """A tile plan that carries nt = 1 (once the packed marker) through the row-major entry
    runs the row-major kernel: the packed kernel is chosen by the entry, not by the plan."""
    x, w, wp, full = _operands(192)
    base, _ = _run(x, w, [1, 3, 0, 2, 64, 128, 1], "none", 1)
    got, _ = _run(x, w, [1, 3, 1, 2, 64, 128, 1], "none", 1)
    assert torch.equal(got, base)
    got, _ = _run(x, wp, [1, 3, 0, 2, 64, 128, 1], "none", 1, packed=True)
    assert torch.equal(got, base)
    _close(base, full, 2e-2, 2e-2)


def test_llama70b_gate_up_mixed_is_bitwise_uniform_on_the_packed_copy():
    """The production case: (64, 57344, 8192, SwiGLU) on the packed copy, 256 wide + 256 narrow
    workgroups, bitwise the uniform 448-tile plan on the row-major weight."""
    M, Nl, K = 64, 57344, 8192
    x, w = _bf(M, K, seed=90), _bf(Nl, K, scale=0.02, seed=91)
    wp = ops.pack_w256(w)
    base = torch.empty(M, Nl // 2, dtype=torch.bfloat16, device=DEV)
    torch.ops.bfly.gemm_with_plan(x, w, base, [1, 3, 0, 2, 64, 128, 1], ops.EPILOGUES["silu"], None)
    got = torch.empty_like(base)
    torch.ops.bfly.gemm_with_plan(x, wp, got, [8, 3, 0, 96, 64, 128, 1], ops.EPILOGUES["silu"], None, None, True)
    assert torch.equal(got, base)
    # as the decode step runs it: behind the row-split RMSNorm (the 1/rms row scale multiplies both
    # SwiGLU factors, so the epilogue's operation order shows), uniform plan against mixed plan
    res = _bf(M, K, seed=93)
    nw = (1.0 + 0.1 * _bf(K, seed=94).float()).to(torch.bfloat16)

    def run(packed):
        xin = ops.rms_norm(x, nw, 1e-5, residual=res.clone(), rows=True)
        return ops.linear(xin, w, epilogue="silu", packed=packed).clone()

    want = _uniform(lambda: run(None))
    assert torch.equal(run(wp), want)     # the default mode: this shape's packed plan is the mixed one
    prev = torch.ops.bfly.gemm_mixed_tiles_mode(2)
    try:
        assert ops.gemm_plan(M, Nl, K)["kind"] == "mixed"
        assert torch.equal(run(None), want)
        assert torch.equal(run(wp), want)
    finally:
        torch.ops.bfly.gemm_mixed_tiles_mode(prev)
