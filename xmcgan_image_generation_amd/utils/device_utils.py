"""Replica groups that share BatchNorm statistics (reference ``xmcgan/utils/device_utils.py:18-26``)."""
from __future__ import annotations


def get_device_groups(group_batch_size, device_batch_size, world):
    """-> the groups as lists of consecutive ranks: ``group_size = group_batch_size // device_batch_size`` replicas each.

    ``world`` stands in for the reference's ``jax.device_count()``.  The reference asserts; a bad combination here is a
    ``ValueError`` that names both numbers."""
    group_batch_size, device_batch_size, world = int(group_batch_size), int(device_batch_size), int(world)
    if group_batch_size <= 0 or device_batch_size <= 0 or world <= 0:
        raise ValueError(f"batch_norm_group_size ({group_batch_size}), the per-device batch ({device_batch_size}) and the "
                         f"number of replicas ({world}) must be positive")
    if group_batch_size % device_batch_size != 0:
        raise ValueError(f"batch_norm_group_size ({group_batch_size}) must be a multiple of the per-device batch "
                         f"({device_batch_size})")
    group_size = group_batch_size // device_batch_size
    if world % group_size != 0:
        raise ValueError(f"the number of replicas ({world}) must be a multiple of the BatchNorm group's replicas "
                         f"({group_size} = batch_norm_group_size {group_batch_size} // per-device batch {device_batch_size})")
    return [list(range(i, i + group_size)) for i in range(0, world, group_size)]


def config_groups(config, world=None):
    """-> (world, device_batch, groups) of ``config.batch_norm_group_size > 0``: world = the initialised process group's size, or
    1, unless given; device_batch = ``config.batch_size // world``, as input_pipeline.create_datasets derives it.  ``ValueError`` where the
    sizes do not fit."""
    import torch.distributed as dist
    if world is None:
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if config.batch_size % world != 0:
        raise ValueError(f"Batch size ({config.batch_size}) must be divisible by the number of devices ({world}).")
    device_batch = config.batch_size // world
    return world, device_batch, get_device_groups(config.batch_norm_group_size, device_batch, world)
