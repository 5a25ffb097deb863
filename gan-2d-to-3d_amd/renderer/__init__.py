"""Mirror of GAN2Shape/renderer/__init__.py."""
from ..plugins.neural_renderer import sweep_shade_torch
from .renderer import Renderer, compose_sweep_pose

__all__ = ["Renderer", "compose_sweep_pose", "sweep_shade_torch"]
