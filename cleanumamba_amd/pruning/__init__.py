"""Structured channel pruning of CleanUMamba (reference: src/pruning/pruninggroup.py, src/pruning/importance.py).

    groups = CleanUMambaPrunableChannels(model)
    chosen, n_params, minima = get_prune_channels(groups, "taylor_squared_individual*n_filters/n_parameters", None,
                                                  0.005, 8, 3e-13)
    prune(groups, chosen, train_step.optimizer)      # or group.prune(indices, optimizer) per group

Importances are computed by one HIP launch for all groups; pruning a model held by a TrainStep keeps its flat
parameter / gradient / Adam buffers, step count, loss scale and hooks (one gather launch), see device.py.
Layer-wise calibration (``layerwise_calibration.calibrator``) measures per-group importance scales with in-place trial
masks instead of pruned deep copies.
"""
from .device import prune
from . import layerwise_calibration
from .importance import calc_importance, get_prune_channels, select_prune_channels
from .pruninggroup import (PC, CleanUMambaPrunableChannels, ParameterContainer, PruningGroup, PruningModule)

__all__ = ["CleanUMambaPrunableChannels", "ParameterContainer", "PC", "PruningGroup", "PruningModule", "calc_importance",
           "get_prune_channels", "select_prune_channels", "prune", "layerwise_calibration"]
