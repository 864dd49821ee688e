"""Name -> factory registry (the slice of the vendored timm registry the trainer uses:
fourm/utils/timm/registry.py:25, fourm/utils/timm/model_builder.py:27-74)."""
_FACTORIES = {}
_UNLISTED = set()          # created by name, not offered by list_models(): the fine-tuning views of fourm.models.fm_vit


def register_model(fn=None, *, listed: bool = True):
    """``listed=False``: found by create_model / is_model / model_entrypoint but left out of ``list_models`` unless asked for, so the
    listing stays the set of pre-training architectures (the trainer's ``--model`` choices)."""
    if fn is None:
        return lambda f: register_model(f, listed=listed)
    _FACTORIES[fn.__name__] = fn
    if not listed:
        _UNLISTED.add(fn.__name__)
    return fn


def is_model(name: str) -> bool:
    return name in _FACTORIES


def model_entrypoint(name: str):
    return _FACTORIES[name]


def list_models(filter: str = "", include_unlisted: bool = False):
    import fnmatch
    names = sorted(n for n in _FACTORIES if include_unlisted or n not in _UNLISTED)
    return fnmatch.filter(names, filter) if filter else names


def create_model(model_name: str, pretrained: bool = False, checkpoint_path: str = "", **kwargs):
    """Look a factory up by name and call it; ``None`` keyword values are dropped (so factories keep
    their defaults), as the upstream builder does."""
    import fourm.models.fm  # noqa: F401  (populates the registry)
    import fourm.models.fm_vit  # noqa: F401
    if not is_model(model_name):
        raise RuntimeError(f"Unknown model ({model_name})")
    kwargs = {k: v for k, v in kwargs.items() if v is not None}
    model = _FACTORIES[model_name](**kwargs)
    if checkpoint_path:
        from .checkpoint import load_state_dict
        model.load_state_dict(load_state_dict(checkpoint_path))
    return model
