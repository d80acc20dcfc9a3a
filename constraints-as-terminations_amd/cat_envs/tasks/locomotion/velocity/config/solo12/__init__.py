"""Task registration (reference: solo12/__init__.py:16-39): same task ids and entry-point keys.
gymnasium's registry is used when it is installed, the package-local one otherwise."""
from cat_envs.shim import register
from cat_envs.tasks.utils.cat.cat_env import CaTEnv

from . import agents

_KW = {
    "clean_rl_cfg_entry_point": f"{agents.__name__}.clean_rl_ppo_cfg:Solo12FlatPPORunnerCfg",
}

register(
    id="Isaac-Velocity-CaT-Flat-Solo12-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12FlatEnvCfg", **_KW},
)

register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Play-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12FlatEnvCfg_PLAY", **_KW},
)

# the same task with the closed-loop servo surrogate as simulator (SyntheticCfg.kind = "servo")
register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoFlatEnvCfg", **_KW},
)

register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-Play-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoFlatEnvCfg_PLAY", **_KW},
)

# the servo task with a RewardsCfg: reward terms evaluated inside the simulator's launch ("Rewards")
register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoRewardsFlatEnvCfg", **_KW},
)

register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-Play-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoRewardsFlatEnvCfg_PLAY", **_KW},
)

# the servo task with an ObservationsCfg: observation terms, scales and noise inside the simulator's launch (DESIGN
# section 9, "Observations"); the play cfg switches the noise off
register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoObsFlatEnvCfg", **_KW},
)

register(
    id="Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-Play-v0",
    entry_point=CaTEnv,
    disable_env_checker=True,
    kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:Solo12ServoObsFlatEnvCfg_PLAY", **_KW},
)

# the servo task with an EventCfg: pushes, reset ranges and traction inside the simulator's launch (DESIGN section 9,
# "Events"); "Full" is rewards, observations and events together.  The play cfgs run with pushes off
for _name, _cfg in (("Events", "Solo12ServoEventsFlatEnvCfg"), ("Full", "Solo12ServoFullFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with a CommandsCfg: the reference's velocity command term inside the simulator's launch (DESIGN section 9,
# "Commands"); "Reference" is rewards, observations, events and commands together
for _name, _cfg in (("Commands", "Solo12ServoCommandsFlatEnvCfg"), ("Reference", "Solo12ServoReferenceFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with a TerminationsCfg: the reference's termination terms inside the simulator's launch (DESIGN section 9,
# "Terminations"); "Reference-Terminations" is these five MDP blocks of the reference's cfg together (the "Reference" task keeps
# its four blocks and its row; the sixth block, the actions, is "Reference-Actions" below)
for _name, _cfg in (("Terminations", "Solo12ServoTerminationsFlatEnvCfg"),
                    ("Reference-Terminations", "Solo12ServoReferenceTerminationsFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with an ActionsCfg: the reference's joint action term inside the simulator's launch (DESIGN section 9,
# "Actions"); "Reference-Actions" is all six MDP blocks of the reference's cfg together (the tasks above keep their rows)
for _name, _cfg in (("Actions", "Solo12ServoActionsFlatEnvCfg"), ("Reference-Actions", "Solo12ServoReferenceActionsFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with a robot: the reference's actuators inside the simulator's launch ("Actuators");
# "Reference-Actuators" is all six MDP blocks and the robot, "DelayedActuators" the same gains behind an actuator delay
for _name, _cfg in (("Actuators", "Solo12ServoActuatorsFlatEnvCfg"), ("Reference-Actuators", "Solo12ServoReferenceActuatorsFlatEnvCfg"),
                    ("DelayedActuators", "Solo12ServoDelayedActuatorsFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with a robot of its own per env: gains, joint friction and base mass drawn inside the simulator's launch
# ("Randomisation"); "Reference-Randomized" is all six MDP blocks, the robot and the three terms
for _name, _cfg in (("Randomized", "Solo12ServoRandomizedFlatEnvCfg"), ("Reference-Randomized", "Solo12ServoReferenceRandomizedFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task with an observation history: the last three frames of every term, kept in the simulator's row by its own
# launch ("History"); "Reference-History" is "Reference-Randomized" behind an actuator delay with that group
for _name, _cfg in (("History", "Solo12ServoHistoryFlatEnvCfg"), ("Reference-History", "Solo12ServoReferenceHistoryFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )

# the servo task under IsaacLab's stock disturbances: a push on the env's own timer and a constant external wrench per episode,
# both inside the simulator's launch ("Disturbances"); "Reference-Disturbances" is all six MDP blocks and the robot
for _name, _cfg in (("Disturbances", "Solo12ServoDisturbancesFlatEnvCfg"),
                    ("Reference-Disturbances", "Solo12ServoReferenceDisturbancesFlatEnvCfg")):
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}", **_KW},
    )
    register(
        id=f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{_name}-Play-v0",
        entry_point=CaTEnv,
        disable_env_checker=True,
        kwargs={"env_cfg_entry_point": f"{__name__}.cat_flat_env_cfg:{_cfg}_PLAY", **_KW},
    )
