from .schedule import KINDS, build_lr_table, check_sgd_options, lr_at, validate_lr_table  # noqa: F401
