"""GPU, one process driving two devices: kernels that ask for more than 64 KiB of dynamic LDS need an opt-in
(hipFuncAttributeMaxDynamicSharedMemorySize) that the HIP runtime keeps per kernel AND per device.  Each case runs on cuda:0 and
then on cuda:1 with identical inputs and must return bit-identical results; a library that remembers the opt-in per process only
never grants it on the second device.  Skipped with fewer than two devices.

Sizes: the smallest that pass through the opt-in.  Two chunks of k_chunk_sort hold 64 KiB of records plus tables, and k_span_pfn
is launched with an 80 000-byte budget, whatever the input.  k_dgrad_s2 at 128 -> 64 channels stages 2 slabs x 9 rows x 34 pixels x
128 B = 78 336 B.  The weight gradient is not here: k_wgrad64 needs 56 032 B (stride 1) / 64 272 B (stride 2), both within the
64 KiB a launch gets without asking, so it cannot show the fault."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def two_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")


def on_both(fn):
    out = []
    for d in (0, 1):
        with torch.cuda.device(d):
            r = fn(torch.device("cuda", d))
            torch.cuda.synchronize()
            out.append([t.cpu() for t in r])
    return out


def test_reader_forward_on_both_devices():
    from pillarnext_amd.reader import PillarFeatureNet

    B, n = 2, 4000
    g = torch.Generator().manual_seed(7)
    pts = torch.empty((n, 6))
    pts[:, 0] = torch.arange(n) // (n // B)  # collated: sorted by sample
    pts[:, 1:3] = torch.rand((n, 2), generator=g) * 27.0 - 13.5  # a few points outside the range
    pts[:, 3] = torch.rand((n,), generator=g) * 5.0 - 2.5
    pts[:, 4:] = torch.rand((n, 2), generator=g)
    torch.manual_seed(11)
    net = PillarFeatureNet(5, [64, 64], [0.2, 0.2, 6], [-12.8, -12.8, -3, 12.8, 12.8, 3])
    with torch.no_grad():
        for pfn in net.pfn_layers:  # non-trivial running statistics
            pfn.norm.running_mean.uniform_(-0.5, 0.5)
            pfn.norm.running_var.uniform_(0.5, 2.0)
            pfn.norm.weight.uniform_(0.5, 1.5)
            pfn.norm.bias.uniform_(-0.5, 0.5)
    state = net.state_dict()

    def run(dev):
        m = PillarFeatureNet(5, [64, 64], [0.2, 0.2, 6], [-12.8, -12.8, -3, 12.8, 12.8, 3])
        m.load_state_dict(state)
        m = m.to(dev).eval()
        counts = torch.zeros((2,), dtype=torch.int32, device=dev)
        canvas = m.forward_dense(pts.to(dev), B, dtype=torch.bfloat16, channels_last=True, counts=counts)
        assert canvas.shape == (B, 64, 128, 128) and canvas.is_contiguous(memory_format=torch.channels_last)
        return canvas.view(torch.int16), counts

    (c0, n0), (c1, n1) = on_both(run)
    assert int(n0[0]) > 1000 and 0 < int(n0[1]) < n  # pillars; kept points (some lie outside)
    assert torch.equal(n0, n1)
    assert torch.equal(c0, c1)
    assert int((c0 != 0).sum()) > 0


def test_masked_dgrad_s2_on_both_devices():
    from pillarnext_amd import ops

    H = W = 32
    g = torch.Generator().manual_seed(5)
    mask_in = (torch.rand((1, H, W), generator=g) < 0.5).to(torch.uint8)
    grad = torch.randn((1, 128, H // 2, W // 2), generator=g)
    w = torch.randn((128, 64, 3, 3), generator=g) * 0.05

    def run(dev):
        gd = grad.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wt = ops.conv3x3_pack_weights(w.to(dev), transposed=True)
        dx = ops.conv3x3_dgrad_s2(gd, wt, 64, (H, W), mask_in.to(dev).contiguous())
        assert dx.shape == (1, 64, H, W)
        return (dx.view(torch.int16),)

    (d0,), (d1,) = on_both(run)
    assert torch.equal(d0, d1)
    assert int((d0 != 0).sum()) > 0
