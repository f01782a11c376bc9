"""training/feeder.py on the device: batches assembled by cum_pcm_batch_f32 against the planned slices, the stale-batch
guard, and a TrainStep fed ``step(batch)`` against one fed the same batches as tensors."""
import copy

import pytest
import torch

import wavtree
from conftest import rel_l2
from test_feeder_host import CROP, LENGTHS, _dataset, expected_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pairs_gpu"))
    return root, wavtree.training_tree(root, LENGTHS, seed=100)


def test_device_batches_equal_the_planned_slices(cuda, tree):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root, pairs = tree
    with BatchFeeder(_dataset(root), 4, cuda, crop_length=CROP, seed=9) as feeder:
        plan = feeder.plan(0)
        assert any(count < CROP for b in plan for _, _, count in b)
        seen = 0
        for batch, entries in zip(feeder, plan):
            assert batch.entries == entries
            clean, noisy = batch.tensors()
            assert clean.device == cuda and clean.dtype == torch.float32 and clean.shape == (4, 1, CROP)
            want_clean, want_noisy = expected_batch(pairs, entries, CROP)
            assert torch.equal(clean.cpu(), want_clean) and torch.equal(noisy.cpu(), want_noisy)
            seen += 1
        assert seen == 3


def test_stale_batch_raises_instead_of_reading_new_data(cuda, tree):
    from cleanumamba_amd.training.feeder import BatchFeeder
    root, pairs = tree
    depth = 2
    with BatchFeeder(_dataset(root), 2, cuda, crop_length=1000, seed=4, depth=depth) as feeder:
        first = feeder.next()
        want = expected_batch(pairs, first.entries, 1000)
        for _ in range(depth - 1):
            feeder.next()
        assert torch.equal(first.tensors()[0].cpu(), want[0])       # depth - 1 further calls: still its own data
        feeder.next()
        with pytest.raises(RuntimeError):
            first.tensors()
        with pytest.raises(RuntimeError):
            first.into(torch.empty(2, 1, 1000, device=cuda), torch.empty(2, 1, 1000, device=cuda))


TINY = dict(channels_input=1, channels_output=1, channels_H=8, max_H=16, encoder_n_layers=3, kernel_size=4, stride=2,
            tsfm_n_layers=2, tsfm_n_head=2, tsfm_d_model=32, tsfm_d_inner=64)


def test_step_fed_a_batch_equals_step_fed_its_tensors(cuda, tmp_path):
    """Two copies of a tiny model, 8 captured steps each on the same feeder batches: one takes ``step(batch)`` (the replay
    assembles into the graph's own inputs), the other ``step(*batch.tensors())``.  Same kernels, same inputs: the bounds
    of test_train_gpu.py::test_graph_replay_equals_eager_steps (parameters rel-L2 < 1e-6, losses 1e-5 relative)."""
    from cleanumamba_amd.network import CleanUMamba
    from cleanumamba_amd.training.feeder import BatchFeeder
    from cleanumamba_amd.training.train_step import TrainStep
    from cleanumamba_amd.util.dataset import CleanNoisyPairDataset
    root = str(tmp_path)
    wavtree.training_tree(root, [9000, 12000, 8000, 16000, 10000, 5000], seed=7)        # one clip is tiled
    torch.manual_seed(0)
    net_a, net_b = CleanUMamba(**TINY), CleanUMamba(**TINY)
    net_b.load_state_dict(copy.deepcopy(net_a.state_dict()), strict=True)
    net_a, net_b = net_a.to(cuda).train(), net_b.to(cuda).train()
    steps = [TrainStep(net_a, optimization={"n_iters": 200}, use_graph=True),
             TrainStep(net_b, optimization={"n_iters": 200}, use_graph=True)]
    losses = [[], []]
    ds = CleanNoisyPairDataset(root=root, subset="training", crop_length_sec=0.5)
    with BatchFeeder(ds, 2, cuda, crop_length=8000, seed=1) as feeder:
        done = 0
        while done < 8:
            for batch in feeder:
                clean, noisy = batch.tensors()
                la, _ = steps[0](batch)
                lb, _ = steps[1](clean, noisy)
                losses[0].append(float(la))
                losses[1].append(float(lb))
                done += 1
                if done == 8:
                    break
        assert steps[0].graph_status == "captured", steps[0].graph_status
        assert steps[1].graph_status == "captured", steps[1].graph_status
        # the last step was a replay: the graph's input is the batch itself
        assert torch.equal(steps[0]._graph["clean"], clean) and torch.equal(steps[0]._graph["noisy"], noisy)
    for (ka, pa), (kb, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert rel_l2(pa, pb) < 1e-6, ka
    assert max(abs(a - b) for a, b in zip(*losses)) < 1e-5 * max(losses[1])
    assert all(l == l for l in losses[0])
