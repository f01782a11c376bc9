"""The streaming runtime's state object (cleanumamba_amd/network/streaming.py) on the CPU: its conversion to and from the
one-launch hop's state blocks (network/hopplan.py), what counts as a live stream, and what a pickled or deep-copied
model carries.  One GPU test at the end checks the same bookkeeping on a stream the one-launch hop really owns.

Reference: CleanUMamba.feed / flush, src/network/CleanUMamba.py:358-490."""
import copy
import pickle

import pytest
import torch

from conftest import load_ckpt, rel_l2


def _net(name, device="cpu"):
    from cleanumamba_amd.network import CleanUMamba
    sd, cfg = load_ckpt(name)
    net = CleanUMamba(**cfg)
    (net.load_state_dict if name == "442k" else net.load_pruned_state_dict)(sd)
    return net.to(device).float().eval()


def _hand_made_state(net, plan, S, g, zero=False):
    """A StreamState as the fused per-layer hop leaves it after a stream's first frame, filled with random values:
    -> (state, the encoder windows (S, C, T) and decoder tails (S, 2, cq) it was made of)."""
    from cleanumamba_amd.network import convstack as cs
    from cleanumamba_amd.network import streaming
    rnd = (lambda *shape: torch.zeros(*shape)) if zero else (lambda *shape: torch.randn(*shape, generator=g))
    st = streaming.StreamState(torch.zeros(S, 0))
    st.params = streaming.new_params(net, S)
    for conv_state, ssm_state in st.params.key_value_memory_dict.values():
        conv_state.copy_(rnd(*conv_state.shape))
        ssm_state.copy_(rnd(*ssm_state.shape))
    windows, tails, T = [], [], net.frame_length
    for i, e in enumerate(plan.encs):
        T = (T - 4) // 2 + 1
        windows.append(rnd(S, e["C"], T))
        st.layers[f"enc{i}"] = cs.to_rows(windows[-1], cs.Geo(S, T, e["C"]), torch.float32)
    for j, d in enumerate(plan.decs):
        tails.append(rnd(S, 2, d["cq"]))
        st.layers[f"dec{j}"] = tails[-1].clone()
    st.input_std, st.frames = 0.5 + rnd(S, 1).abs(), 1
    return st, windows, tails


@pytest.mark.parametrize("name", ["442k", "pruned500k"])
def test_state_round_trips_through_the_hop_kernels_block(name):
    """import_state -> export_rows / export_state give back, bit for bit, what the drain reads of a hand-made state: the
    rows of every encoder window no hop has consumed, the decoder tails channels-first, the Mamba states; the block's
    header holds the running std and a frame count of 1."""
    from cleanumamba_amd.network import hopplan
    net = _net(name)
    net.normalize_input = True
    plan = hopplan.HopPlan(net)
    S = 3
    st, windows, tails = _hand_made_state(net, plan, S, torch.Generator().manual_seed(11))
    block = plan.import_state(st)
    assert block.shape == (S, plan.state_stride)
    assert torch.equal(block[:, 0:1], st.input_std) and torch.equal(block[:, 1], torch.ones(S))
    rows = plan.export_rows(block)
    for i, e in enumerate(plan.encs):
        assert torch.equal(rows[f"enc{i}"], windows[i][:, :, e["n"]:])
    for j, d in enumerate(plan.decs):
        assert rows[f"dec{j}"].shape == (S, d["cout"], 2)
        assert torch.equal(rows[f"dec{j}"], tails[j][:, :, :d["cout"]].transpose(1, 2))
    # into rows `at` of a larger block, as a stream pool imports its first frames
    big = torch.zeros(5, plan.state_stride)
    plan.import_state(st, into=big, at=torch.tensor([4, 0, 2]))
    assert torch.equal(big[[4, 0, 2]], block) and not big[[1, 3]].any()
    other, _, _ = _hand_made_state(net, plan, S, None, zero=True)
    again = plan.export_state(other, block)
    assert all(torch.equal(again[k], rows[k]) for k in rows)
    kv, kv0 = other.params.key_value_memory_dict, st.params.key_value_memory_dict
    assert len(kv) == len(plan.blks) == len(kv0)
    for k in kv0:
        assert kv0[k][0].abs().sum() > 0 and kv0[k][1].abs().sum() > 0
        assert torch.equal(kv[k][0], kv0[k][0]) and torch.equal(kv[k][1], kv0[k][1])


def _live_cases():
    """(what makes the stream live, a function that puts it there), on hand-made states: no hop runs."""
    def pending(st):
        st.pending = torch.zeros(2, 5)

    def layers(st):
        st.layers["enc0"] = torch.zeros(2, 4, 6)

    def kernel(st):
        st.kernel = {"plan": None, "state": None, "plan_weights": None}
    return [("pending samples", pending), ("per-layer buffers", layers), ("a kernel-owned state", kernel)]


def test_live_and_refuse_live_streams():
    from cleanumamba_amd.pruning.device import refuse_live_streams
    net = _net("pruned500k")
    assert not net.stream.live
    refuse_live_streams([net], "prune", "pruning")
    for what, make in _live_cases():
        net.reset_stream()
        assert not net.stream.live, what
        make(net.stream.state)
        assert net.stream.live, what
        with pytest.raises(RuntimeError, match="live stream"):
            refuse_live_streams([net], "prune", "pruning")
    net.reset_stream()
    assert not net.stream.live
    refuse_live_streams([net], "prune", "pruning")


@pytest.mark.parametrize("clone", [copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m))], ids=["deepcopy", "pickle"])
def test_copies_keep_a_per_layer_stream_and_restart_a_kernel_owned_one(clone):
    from cleanumamba_amd.network import hopplan
    net = _net("pruned500k")
    plan = hopplan.HopPlan(net)
    st, _, _ = _hand_made_state(net, plan, 2, torch.Generator().manual_seed(5))
    st.pending = torch.randn(2, 37, generator=torch.Generator().manual_seed(6))
    st.graph = {"failed": True, "error": "a graph record"}
    st.wv = (1, True)
    net.stream.state = st
    net.stream.why = "asked"
    net.__dict__["_hop_plan"] = ((1, True), plan)
    twin = clone(net)
    ts = twin.stream.state
    assert ts is not st and twin.stream.live
    assert torch.equal(ts.pending, st.pending) and ts.frames == 1 and torch.equal(ts.input_std, st.input_std)
    assert sorted(ts.layers) == sorted(st.layers) and all(torch.equal(ts.layers[k], st.layers[k]) for k in st.layers)
    for k, (conv_state, ssm_state) in st.params.key_value_memory_dict.items():
        assert torch.equal(ts.params.key_value_memory_dict[k][0], conv_state)
        assert torch.equal(ts.params.key_value_memory_dict[k][1], ssm_state)
    assert ts.graph is None and ts.kernel is None and ts.wv is None and twin.stream.why is None
    assert "_hop_plan" not in twin.__dict__ and "_hop_plan" in net.__dict__
    assert st.graph is not None and net.stream.why == "asked"              # (the original is left as it was)
    # the one-launch hop owns the stream: its state lives in device blocks no copy carries -- the copy starts afresh
    st.kernel = {"plan": plan, "state": torch.zeros(2, plan.state_stride), "plan_weights": (1, True)}
    twin = clone(net)
    ts = twin.stream.state
    assert not twin.stream.live and ts.kernel is None and ts.graph is None
    assert ts.pending.shape == (2, 0) and ts.layers == {} and ts.frames == 0 and ts.params is None and ts.input_std == 0
    assert "_hop_plan" not in twin.__dict__
    assert net.stream.live and net.stream.state.kernel is not None


@pytest.mark.gpu
def test_kernel_owned_stream_bookkeeping(cuda):
    """A stream the one-launch hop owns: where its records live, what a pickled copy does with it, what flush leaves."""
    net = _net("pruned500k", cuda)
    assert net.normalize_input
    S, n = 2, net.frame_length + 3 * net.total_stride
    g = torch.Generator().manual_seed(21)
    clip1 = (0.3 * torch.randn(S, n, generator=g)).to(cuda)
    clip2 = (0.02 * torch.randn(S, n, generator=g)).to(cuda)
    with torch.no_grad():
        out = net.feed_batch(clip1)
        assert out.shape == (S, 4 * net.total_stride)
        assert net.hop_kernel_status == "active"
        assert net.__dict__["_hop_plan"][1].flops_per_hop > 0
        # the plan cache is the one streaming record kept in the model's own dict (the benchmark reads it there)
        assert {k for k in net.__dict__ if k.startswith(("_hop", "_wv", "_pl"))} == {"_hop_plan"}
        assert net.stream.live
        twin, fresh = pickle.loads(pickle.dumps(net)), _net("pruned500k", cuda)
        assert not twin.stream.live and twin.hop_kernel_status == "first frame pending"
        a = torch.cat([twin.feed_batch(clip2), twin.flush_batch()], 1)
        b = torch.cat([fresh.feed_batch(clip2), fresh.flush_batch()], 1)
        assert a.shape == b.shape == (S, n)
        assert rel_l2(a, b) < 1e-6                      # (tolerance of test_stream_after_flush_starts_a_fresh_running_std)
        tail = net.flush_batch()
        assert tail.shape == (S, n - 4 * net.total_stride)
    assert not net.stream.live and net.hop_kernel_status == "first frame pending"
    assert net.__dict__["_hop_plan"][1].flops_per_hop > 0
