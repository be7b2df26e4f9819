"""k_epoch_draw on the GPU against the restatement of its stated function (tests/epoch_draw_reference.py), bit for bit; then one
recorded draw replayed three times against three eager draws of the restatement."""
import pytest
import torch

from epoch_draw_reference import case, epoch_draw

pytestmark = pytest.mark.gpu

CASES = [(5, 3, 2, 1), (33, 8, 32, 7), (1000, 8, 7, 7), (1025, 31, 1024, 30)]          # (n_images, K, B, num_neighbors)
POISON = -0x0101010101010102                                                          # no index, no count


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.mark.parametrize("n,K,B,nn", CASES, ids=[f"n{c[0]}-K{c[1]}-B{c[2]}-nn{c[3]}" for c in CASES])
def test_kernel_matches_the_restatement(n, K, B, nn, dev):
    """Three consecutive calls: the cursor and `draws` advance on the device (`draws` across 2^32: the counter's second word).  Outputs
    are poisoned in front of every call, and so are the words beside the state and the outputs: every element is written, nothing else."""
    from depthg_amd import ops
    order, nns = case(n, K)
    order_d, nns_d = order.to(dev), nns.to(dev)
    first = [0x1234567887654321, 2 ** 32 - 3, 0]
    state_buf = torch.full((5,), POISON, dtype=torch.int64, device=dev)
    state = state_buf[1:4]
    state.copy_(torch.tensor(first))
    want_state = first
    for call in range(3):                                        # (the largest case runs past the end: the held position)
        out = torch.full((2 * B + 3,), POISON, dtype=torch.int64, device=dev)
        ind, ind_pos = out[1:B + 1], out[B + 2:2 * B + 2]
        a, b = ops.epoch_draw(state, order_d, nns_d, B, nn, ind, ind_pos)
        assert a is ind and b is ind_pos
        want_ind, want_pos, want_state = epoch_draw(want_state, order.tolist(), nns.tolist(), B, nn)
        got = out.cpu()
        assert got[1:B + 1].tolist() == want_ind, f"ind of call {call}"
        assert got[B + 2:2 * B + 2].tolist() == want_pos, f"ind_pos of call {call}"
        assert got[0] == got[B + 1] == got[2 * B + 2] == POISON
        assert state_buf.cpu().tolist() == [POISON] + want_state + [POISON], f"state after call {call}"
        assert all(p in nns[i, 1:nn + 1].tolist() for i, p in zip(want_ind, want_pos))
    assert torch.equal(order_d.cpu(), order) and torch.equal(nns_d.cpu(), nns)


def test_fresh_buffers_and_the_host_refusals(dev):
    from depthg_amd import ops
    order, nns = case(40, 6)
    state = torch.tensor([7, 0, 0], dtype=torch.int64, device=dev)
    ind, ind_pos = ops.epoch_draw(state, order.to(dev), nns.to(dev), 8, 5)
    want_ind, want_pos, want_state = epoch_draw([7, 0, 0], order.tolist(), nns.tolist(), 8, 5)
    assert ind.tolist() == want_ind and ind_pos.tolist() == want_pos and state.tolist() == want_state
    with pytest.raises(ValueError, match="on cuda"):
        ops.epoch_draw(state, order, nns.to(dev), 8, 5)          # (an operand elsewhere)
    assert state.tolist() == want_state


def test_a_recorded_draw_draws_anew_at_every_replay(dev):
    """DeviceEpoch.draw() recorded once, replayed three times: the three results are three eager draws of the restatement - the seed,
    the draw count and the cursor are read from the device, nothing is baked into the graph."""
    from depthg_amd.epoch import DeviceEpoch
    n, K, B, nn = 64, 9, 16, 7
    _, nns = case(n, K)
    ep = DeviceEpoch(nns, B, nn, dev, shuffle=True, generator=torch.Generator().manual_seed(3))
    ep.begin_epoch()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ep.draw()                                                # (warm-up: one eager draw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_state = ep.state.tolist()
    assert want_state[1:] == [B, B]
    order = ep.order.tolist()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ind, ind_pos = ep.draw()
    assert ind is ep.ind and ind_pos is ep.ind_pos
    assert ep.state.tolist() == want_state, "recording must not execute anything"
    results = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want_ind, want_pos, want_state = epoch_draw(want_state, order, nns.tolist(), B, nn)
        assert ind.tolist() == want_ind and ind_pos.tolist() == want_pos and ep.state.tolist() == want_state
        results.append((want_ind, want_pos))
    assert results[0] != results[1] != results[2]
    assert sum((r[0] for r in results), []) == order[B:4 * B]
