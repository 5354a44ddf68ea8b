"""dagr_gemm_epilogue (csrc/gemm_lt.hip: the image branch's 1x1 convolutions as library GEMMs with bias, residual and ReLU
in the epilogue) called directly, and the check that the engine really runs it.

Bar, elementwise against float64 (tests/kernel_refs.py):
    |got - act(A64 @ W64 + b + R)| <= (K + 3) * 2^-24 * (|A| @ |W| + |b| + |R|)
the worst-case bound of an fp32 dot product of K terms plus the two epilogue adds in ANY summation order, with or without
FMA (every partial sum is bounded by the magnitude on the right and is rounded at most K + 2 times at 2^-24; second-order
terms are covered by the spare 2^-24).  It is derived, not tuned: a result outside it means the library chose a kernel
that does not accumulate in fp32."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
UNSUPPORTED = -4      # DAGR_ERR_UNSUPPORTED


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, ld, fill=SENTINEL):
    """a[M, n] as the leading columns of a [M, ld] matrix."""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


def _workspace():
    n = int(_lib.lib().dagr_gemm_epilogue_workspace_bytes())
    if _workspace.t is None:
        _workspace.t = torch.empty(n, dtype=torch.uint8, device="cuda")
    return _workspace.t


_workspace.t = None


def _operands(M, K, N, bias, res, seed):
    r = np.random.default_rng(seed)
    A = r.standard_normal((M, K), dtype=np.float32)
    W = (r.standard_normal((K, N), dtype=np.float32) / np.float32(np.sqrt(K))).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) if bias else None
    R = r.standard_normal((M, N), dtype=np.float32) if res else None
    return A, W, b, R


def _call(A, W, b, R, act, lda=None, ldr=None, ldd=None):
    """Runs the entry on device copies (A and R padded to their leading dimensions) and checks that it wrote none of its
    inputs; returns (rc, D[M, ldd]), D pre-filled with the sentinel."""
    M, K = A.shape
    N = W.shape[1]
    lda, ldr, ldd = lda or K, ldr or N, ldd or N
    hA = _padded(A, lda)
    hR = None if R is None else _padded(R, ldr)
    dA, dW, db, dR = _dev(hA), _dev(W), _dev(b), _dev(hR)
    dD = torch.full((M, ldd), SENTINEL, dtype=torch.float32, device="cuda")
    ws = _workspace()
    rc = _lib.lib().dagr_gemm_epilogue(_lib.ptr(dA), M, K, lda, _lib.ptr(dW), N, _lib.ptr(db), _lib.ptr(dR), ldr, act,
                                       _lib.ptr(dD), ldd, _lib.ptr(ws), ws.numel(), _lib.cur_stream(torch.device("cuda:0")))
    torch.cuda.synchronize()
    for d, h in ((dA, hA), (dW, W), (db, b), (dR, hR)):
        if d is not None:
            assert np.array_equal(d.cpu().numpy(), h), "an input was written"
    return rc, dD.cpu().numpy()


def _assert_within_bound(got, A, W, b, R, act, what=""):
    K = A.shape[1]
    ref, mag = kr.gemm_epilogue(A, W, b, R, act)
    err = np.abs(got - ref)
    bound = (K + 3) * 2.0 ** -24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"gemm_epilogue {what}: max |err| / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: max |err| / bound = {worst}"


def _last_error():
    return _lib.lib().dagr_last_error().decode("utf-8", "replace")


SHAPES = [(1, 64, 64), (7, 64, 256), (129, 256, 64), (1000, 512, 128), (333, 2048, 512), (8640, 64, 256)]
ENGINE_COMBOS = [(True, False, 1), (True, True, 1), (True, False, 0)]     # bias + ReLU, bias + R + ReLU, bias only


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bias,res,act", ENGINE_COMBOS)
def test_the_engines_three_epilogues_on_every_shape(shape, bias, res, act):
    M, K, N = shape
    A, W, b, R = _operands(M, K, N, bias, res, seed=M + K + N)
    rc, D = _call(A, W, b, R, act)
    assert rc == 0, _last_error()
    _assert_within_bound(D, A, W, b, R, act, f"{shape} bias={bias} R={res} act={act}")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_all_eight_epilogues(bias, res, act):
    M, K, N = 129, 256, 64
    A, W, b, R = _operands(M, K, N, bias, res, seed=17)
    rc, D = _call(A, W, b, R, act)
    assert rc == 0, _last_error()
    _assert_within_bound(D, A, W, b, R, act, f"bias={bias} R={res} act={act}")
    if act:
        assert (D == 0).any() and (D > 0).any()
    else:
        assert (D < 0).any()


def test_padded_leading_dimensions_and_untouched_padding():
    M, K, N = 129, 256, 64
    A, W, b, R = _operands(M, K, N, True, True, seed=23)
    rc, D = _call(A, W, b, R, 1, lda=K + 4, ldr=N + 4, ldd=N + 8)
    assert rc == 0, _last_error()
    assert D.shape == (M, N + 8) and np.all(D[:, N:] == SENTINEL), "the padding columns of D were written"
    _assert_within_bound(D[:, :N], A, W, b, R, 1, "padded lda / ldr / ldd")


def test_a_cached_plan_follows_new_operands():
    """One key (shape, strides, epilogue) four times, every time with buffers of its own: the plan made by the first call
    -- which also times the library's candidates on that call's operands -- must read the later calls' A, bias and R and
    write their D."""
    M, K, N = 131, 256, 64          # a key no other test of this file uses: the first call here is the planning one
    first = _operands(M, K, N, True, True, seed=31)
    rc, D1 = _call(*first, 1)
    assert rc == 0, _last_error()
    _assert_within_bound(D1, *first, 1, "planning call")
    rc, D2 = _call(*first, 1)       # the same data in new buffers
    assert rc == 0, _last_error()
    assert np.array_equal(D1.view(np.int32), D2.view(np.int32)), "same data, same plan, different bits"
    for seed in (32, 33):
        ops = _operands(M, K, N, True, True, seed=seed)
        ops = (ops[0], first[1], ops[2], ops[3])        # the layer's weights stay, as in the engine
        rc, D = _call(*ops, 1)
        assert rc == 0, _last_error()
        _assert_within_bound(D, *ops, 1, f"cached plan, operands {seed}")
        assert not np.array_equal(D, D1)


def test_odd_shape_is_right_or_refused():
    """(5, 3, 7): rows that are no multiple of 16 bytes.  Either the library has a kernel and the result is inside the bar,
    or the entry says DAGR_ERR_UNSUPPORTED; never 0 with a wrong result."""
    M, K, N = 5, 3, 7
    A, W, b, R = _operands(M, K, N, True, True, seed=41)
    rc, D = _call(A, W, b, R, 1)
    assert rc in (0, UNSUPPORTED), _last_error()
    if rc == 0:
        _assert_within_bound(D, A, W, b, R, 1, "odd shape")


# ------------------------------------------------------------------------------------------------ which path runs
@pytest.mark.parametrize("img_net", ["resnet50", "resnet18"])
def test_the_engine_runs_the_fused_gemm_and_its_torch_fallback_agrees(img_net, monkeypatch):
    """_Conv1x1Gemm.forward drops to torch for good after one non-zero return of dagr_gemm_epilogue.  After a whole image
    branch the switch must still be on (so the fused GEMM is what ran, and what bench.py times); with the switch off the
    same maps must come out within the image-branch test's own bar."""
    from dagr_amd import engine
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils.testing_weights import randomize_
    from oracle import model as om

    W, H, B = 320, 215, 2
    torch.manual_seed(8)
    args = om.default_args(batch_size=B, use_image=True, img_net=img_net)
    model = randomize_(DAGR(args, height=H, width=W), seed=8).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    eng = model.engine()
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    assert engine._LT["ok"] is True, "the fused GEMM was already switched off before this test"
    with torch.no_grad():
        feats, cnn = eng._image_branch(image)
        torch.cuda.synchronize()
        assert any(isinstance(m, engine._Conv1x1Gemm) for m in eng._net_f.modules())
        feats = [f.clone() for f in feats]
        cnn = {k: [t.clone() for t in v] for k, v in cnn.items()}
        assert engine._LT["ok"] is True, f"dagr_gemm_epilogue failed inside the image branch: {_last_error()}"
        monkeypatch.setitem(engine._LT, "ok", False)
        feats_t, cnn_t = eng._image_branch(image)
        torch.cuda.synchronize()
    pairs = list(zip(feats, feats_t)) + [(a, b) for k in cnn_t for a, b in zip(cnn[k], cnn_t[k])]
    assert len(pairs) > len(feats)
    for a, b in pairs:
        assert float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))
