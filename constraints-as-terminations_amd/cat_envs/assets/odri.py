"""Configuration of the ODRI Solo12 for the servo task (the reference's ``cat_envs.assets.odri`` path).

* :obj:`SOLO12_CFG`: the Solo12 with the reference's actuators - one ideal PD group over all twelve joints, stiffness 4,
  damping 0.2, armature 0.00036207, effort limit 10 Nm, velocity limit 100 rad/s - and its default joint positions
* :obj:`SOLO12_MINIMAL_CFG`: the same robot (the reference's variant with minimal collision bodies; the surrogate has none)

``spawn`` stays unset: there is no USD stage here.  Only ``actuators`` and ``init_state.joint_pos`` are read
(``cat_envs.tasks.utils.mdp.actuators.build_table``).
"""
from cat_envs.shim import ArticulationCfg, IdealPDActuatorCfg

_LEGS = ("FL", "FR", "HR", "HL")
_LEFT = ("FL", "HL")

SOLO12_CFG = ArticulationCfg(
    init_state=ArticulationCfg.InitialStateCfg(
        pos=(0.0, 0.0, 0.3),
        joint_pos={**{f"{leg}_HAA": 0.05 if leg in _LEFT else -0.05 for leg in _LEGS},
                   **{f"{leg}_HFE": 0.4 for leg in _LEGS}, **{f"{leg}_KFE": -0.8 for leg in _LEGS}},
        joint_vel={".*": 0.0},
    ),
    soft_joint_pos_limit_factor=1.0,
    actuators={
        "legs": IdealPDActuatorCfg(
            joint_names_expr=[f"{leg}_{part}" for leg in _LEGS for part in ("HAA", "HFE", "KFE")],
            armature=0.00036207,
            effort_limit=10.0,
            velocity_limit=100.0,
            stiffness={".*": 4.0},
            damping={".*": 0.2},
        ),
    },
)
SOLO12_MINIMAL_CFG = SOLO12_CFG.copy()
