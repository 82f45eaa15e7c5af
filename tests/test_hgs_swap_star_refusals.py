"""What the SWAP* surface refuses, and the polar angles it feeds the kernel (engine.hgs_polar_angles)."""
import ctypes as C

import pytest
import torch


def test_swap_star_without_positions_raises():
    from deepaco_amd import engine
    from deepaco_amd.cvrp_nls.aco import ACO
    paths = torch.zeros((1, 8, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="positions"):
        engine.hgs_local_search_(paths, [], torch.zeros(4), use_swap_star=True)
    d = torch.rand(5, 5, dtype=torch.double)
    with pytest.raises(ValueError, match="positions"):
        engine.BatchedCVRP(d[None], torch.zeros(1, 5), local_search="hgs", use_swap_star=True)
    with pytest.raises(ValueError, match="positions"):
        ACO(d, torch.zeros(5, dtype=torch.double), use_swap_star=True)


def test_polar_angles_of_the_axes_and_diagonals():
    """libm's atan2 is exact in the sense needed on the axes and diagonals: k * pi / 4 rounded to nearest, and
    32768 * that / 3.14159265359 lies just below k * 8192 (HGS's constant is above pi), so truncation decides: by hand,
      east 0 -> 0;  north-east pi/4 -> 8191.99.. -> 8191;  north pi/2 -> 16383;  north-west 3pi/4 -> 24575;  west pi -> 32767;
      south-west -3pi/4 -> -24575 -> 40961;  south -pi/2 -> -16383 -> 49153;  south-east -pi/4 -> -8191 -> 57345;
    the node at the depot's own position: atan2(0, 0) = 0 -> 0."""
    from deepaco_amd import engine
    pos = torch.tensor([[2.0, 3.0], [3.0, 3.0], [3.0, 4.0], [2.0, 4.0], [1.0, 4.0], [1.0, 3.0], [1.0, 2.0], [2.0, 2.0], [3.0, 2.0], [2.0, 3.0]],
                       dtype=torch.float64)
    want = [0, 0, 8191, 16383, 24575, 32767, 40961, 49153, 57345, 0]
    got = engine.hgs_polar_angles(pos)
    assert got.dtype == torch.int32 and got.tolist() == want
    both = engine.hgs_polar_angles(torch.stack((pos, pos.flip(0))))
    assert both.shape == (2, 10) and both[0].tolist() == want and both[1, 0].item() == 0


@pytest.mark.gpu
def test_bad_arguments_return_the_error_codes():
    from deepaco_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, A, Lmax, g = 20, 4, 30, 20
    wsb = _lib.lib().daco_hgs_workspace_bytes_ss(1, n, A, Lmax, g)
    buf = torch.zeros(max(wsb, 1 << 20), dtype=torch.uint8, device=dev)
    P = buf.data_ptr()
    one = (C.c_void_p * 1)(P)
    strides, counts = (C.c_long * 1)(n * n), (C.c_int * 1)(1)
    assert 0 < wsb <= buf.numel()

    def call(n_=n, xy=P, polar=P):
        return L.daco_hgs_local_search_ss(None, 1, n_, A, Lmax, 1, one, None, strides, one, counts, P, 1000.001, g, P, P, None, P, buf.numel(), xy, polar)

    assert call(xy=None) == -1 and b"xy" in L.daco_last_error()
    assert call(polar=None) == -1 and b"polar" in L.daco_last_error()
    assert call(n_=16001) == -2 and b"16000" in L.daco_last_error()
    with pytest.raises(_lib.DacoTooLarge):
        _lib.check(call(n_=16001), "daco_hgs_local_search_ss")
