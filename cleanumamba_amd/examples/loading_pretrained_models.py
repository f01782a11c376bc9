"""Load a released checkpoint -- interface of src/examples/loading_pretrained_models.py:7-19."""
import torch

from ..network.network import Net


def load_pretrained_CleanUMamba(path="checkpoints/models/CleanUMamba-3N-E8-high.pkl"):
    """The model of a checkpoint file holding ``network_config`` and ``model_state_dict``, on the GPU in float32.  Built
    as the reference builds it: ``Net("CleanUMamba", config)`` with ``device = "cuda"``, then ``load_pruned_state_dict``
    (every parameter takes the checkpoint's shape, so pruned and unpruned checkpoints load alike), ``.cuda().float()``."""
    checkpoint = torch.load(path, map_location="cpu")
    config = dict(checkpoint["network_config"])
    config["device"] = "cuda"
    model = Net("CleanUMamba", config)
    if hasattr(model, "load_pruned_state_dict") and callable(model.load_pruned_state_dict):
        model.load_pruned_state_dict(checkpoint["model_state_dict"])
    else:
        model.load_state_dict(checkpoint["model_state_dict"])
    model.cuda()
    model.float()
    return model
