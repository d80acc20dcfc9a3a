"""Robot configurations of the servo task (the reference's ``cat_envs.assets`` path)."""
from .odri import SOLO12_CFG, SOLO12_MINIMAL_CFG  # noqa: F401
