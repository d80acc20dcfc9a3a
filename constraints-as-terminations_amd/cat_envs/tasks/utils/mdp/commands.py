"""Command terms of the servo task (the reference's ``mdp/commands.py`` path; DESIGN section 9, "Commands").

``UniformVelocityCommandCfg`` carries the field names of IsaacLab's ``isaaclab.envs.mdp.UniformVelocityCommandCfg``,
``UniformVelocityCommandWithDeadzoneCfg`` those of the reference's subclass - PARITY UNPINNED: the rules are restated from
the reference's ``_update_command`` and IsaacLab's published form, IsaacLab is not installed next to this package and
nothing here is compared with it.

No term does anything in Python.  The command manager turns the cfg into the 16-word block the simulator's kernel reads
inside its own launch (include/catppo.h, catppo_servo_commands).  What the two classes mean there:

* ``UniformVelocityCommandCfg``: a new command every ``resampling_time_range`` seconds, uniform in ``ranges``; a share
  ``rel_standing_envs`` of the draws stands still (flag STANDING).
* ``UniformVelocityCommandWithDeadzoneCfg``: the reference's override.  Every step a command with no component above
  ``velocity_deadzone`` becomes zero, a standing robot gets a new command with probability 0.01 and a moving one with
  ``physics_dt / max_episode_length_s``, and the yaw command flips sign at that same rate (flags DEADZONE,
  RANDOM_RESAMPLE, YAW_FLIP).  ``rel_standing_envs`` is accepted and inert: the override never applies it.
"""
from __future__ import annotations

from cat_envs.shim import MISSING, configclass


@configclass
class Ranges:
    """uniform ranges (lo, hi) of the three commands [m/s, m/s, rad/s]"""
    lin_vel_x: tuple = MISSING
    lin_vel_y: tuple = MISSING
    ang_vel_z: tuple = MISSING
    heading: tuple = None                          # inert: the model has no heading


@configclass
class UniformVelocityCommandCfg:
    asset_name: str = "robot"
    resampling_time_range: tuple = MISSING         # (lo, hi) seconds between two timed resamples
    heading_command: bool = False                  # True is an error: the model has no heading
    heading_control_stiffness: float = 1.0         # inert
    rel_standing_envs: float = 0.0
    rel_heading_envs: float = 1.0                  # inert
    debug_vis: bool = False                        # inert
    ranges: Ranges = MISSING


# the Ranges class under IsaacLab's name, UniformVelocityCommandCfg.Ranges
UniformVelocityCommandCfg.Ranges = Ranges


@configclass
class UniformVelocityCommandWithDeadzoneCfg(UniformVelocityCommandCfg):
    velocity_deadzone: float = 0.1
    #: optional overrides of the two resampling probabilities (tests, robustness runs); None: 0.01 and
    #: ``sim.dt / episode_length_s``, the reference's
    p_still: float = None
    p_move: float = None
