"""The configuration a command runs with: one yml file, or the merge of the reference's command line
(main.py:69-81) — `minimal_config.yml` overlaid with `configs/<category>.yml`."""
import os


def _read(path):
    import yaml
    if not os.path.isfile(path):
        raise FileNotFoundError(f"config file {path!r} not found")
    with open(path) as f:
        config = yaml.safe_load(f)
    if config is None:
        return {}
    if not isinstance(config, dict):
        raise ValueError(f"config file {path!r} does not hold a mapping of keys")
    return config


def load_config(config_file=None, category=None, config_dir="."):
    """With `category`: <config_dir>/minimal_config.yml overlaid with <config_dir>/configs/<category>.yml (keys of the
    second file win) and config["category"] = category.  Otherwise the one file `config_file`.  A missing file raises
    FileNotFoundError naming the path."""
    if category is not None:
        config = {**_read(os.path.join(config_dir, "minimal_config.yml")),
                  **_read(os.path.join(config_dir, "configs", f"{category}.yml"))}
        config["category"] = category
        return config
    if config_file is None:
        raise ValueError("load_config needs config_file or category")
    return _read(config_file)
