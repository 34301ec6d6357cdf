"""MI355X-native vectorised MARL responsible-navigation grid world (host side)."""


def __getattr__(name):  # marlnav.resp_map_from_counts / marlnav.resp_table, imported on first use
    if name in ("resp_map_from_counts", "resp_table"):
        from . import resp_map
        return getattr(resp_map, name)
    if name == "resp_footprint_from_counts":
        from . import resp_footprint
        return resp_footprint.resp_footprint_from_counts
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
