"""openpystruct_amd -- MI355X-native batched beam FE solve (the OpenPyStruct data-generation hot path).

Host side in Python over a C-ABI HIP library; see DESIGN.md and INTEGRATION.md.
"""
from . import runtime  # noqa: F401  (entry points call runtime.configure() before their first HIP call; importing sets nothing)
from .beam import BeamSolution, beam_solve, beam_solve_vjp, differentiable_beam_solve, kernel_name  # noqa: F401
from .frames import (FrameCaseSolution, FrameFactor, differentiable_frame_solve, frame_dataset_draws, frame_element_load_vjp,  # noqa: F401
                     frame_factor, frame_resolve, frame_sizing_gradient, frame_solve_cases, frame_solve_cases_vjp, frame_solve_vjp,
                     generate_frame_dataset, grid_load_cases)
from .sizing import GRADIENTS, beam_sizing_gradient  # noqa: F401
from .multicase import generate_multicase_dataset, optimize_designs  # noqa: F401
from .frame_designs import FrameDesigns, frame_design_gradient, generate_frame_design_dataset, optimize_frame_designs  # noqa: F401
from .frame_groups import (DiscreteDesigns, FrameDesignValues, GroupedFrameDesigns, MemberGroups, evaluate_frame_designs,  # noqa: F401
                           frame_group_gradient, generate_grouped_frame_design_dataset, member_groups, optimize_grouped_frame_designs,
                           snap_to_catalogue, story_groups)
from .design_loss import DesignObjective, design_gap, design_objective, design_objective_term  # noqa: F401
from .frame_modes import (FrameMass, FrameModes, differentiable_frame_frequencies, frame_modes, frame_modes_vjp,  # noqa: F401
                          frame_solve_modes)
from .frame_buckling import (FrameBuckling, differentiable_frame_buckling, frame_buckling, frame_buckling_vjp,  # noqa: F401
                             frame_solve_buckling)
from .frame_frequency import FrequencyFloor  # noqa: F401
from . import torch_op  # noqa: F401  (registers torch.ops.openpystruct_amd.beam_solve / frame_solve, their VJP ops and autograd formulas)

__all__ = ["BeamSolution", "beam_solve", "beam_solve_vjp", "differentiable_beam_solve", "kernel_name",
           "frame_solve_vjp", "differentiable_frame_solve", "GRADIENTS", "beam_sizing_gradient", "frame_sizing_gradient",
           "frame_element_load_vjp", "grid_load_cases", "frame_dataset_draws", "generate_frame_dataset", "optimize_designs",
           "generate_multicase_dataset", "FrameFactor", "FrameCaseSolution", "frame_factor", "frame_resolve", "frame_solve_cases",
           "frame_solve_cases_vjp", "FrameDesigns", "optimize_frame_designs", "frame_design_gradient", "generate_frame_design_dataset",
           "DesignObjective", "design_objective", "design_objective_term", "design_gap", "MemberGroups", "member_groups", "story_groups",
           "GroupedFrameDesigns", "DiscreteDesigns", "FrameDesignValues", "optimize_grouped_frame_designs", "frame_group_gradient",
           "evaluate_frame_designs", "snap_to_catalogue", "generate_grouped_frame_design_dataset", "FrameMass", "FrameModes", "frame_modes",
           "frame_solve_modes", "frame_modes_vjp", "differentiable_frame_frequencies", "FrameBuckling", "frame_buckling", "frame_solve_buckling",
           "frame_buckling_vjp", "differentiable_frame_buckling", "FrequencyFloor"]
