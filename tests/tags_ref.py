"""The expectation of tsdbhip_regroup_tags, in plain Python over dicts and sets: which series a
tag query sees, the group key of each, and the keys' dense numbering in ByteMap order (DESIGN.md
5.18).  It never uses the engine.

A tag query is (filters, group_by, explicit_tags) or an object with filter_list / group_by_list /
explicit_tags (abi.HostTagQuery): filters are (tagk uid, kind, tagv uids), kind one of ANY / IN /
NOT_IN / NOT_KEY below; group_by the tagk uids in ascending order."""
from __future__ import annotations

ANY, IN, NOT_IN, NOT_KEY = 0, 1, 2, 3
GROUP_NONE, GROUP_EXCLUDED = -1, -2


def parts(tag_query):
    if hasattr(tag_query, "filter_list"):
        return tag_query.filter_list, tag_query.group_by_list, tag_query.explicit_tags
    filters, group_by, explicit = tag_query
    return filters, group_by, explicit


def holds(kind, tags: dict, tagk, values) -> bool:
    """One primitive, a pure predicate on a series' tag map."""
    if kind == ANY:
        return tagk in tags
    if kind == IN:
        return tagk in tags and tags[tagk] in values
    if kind == NOT_IN:
        return tagk not in tags or tags[tagk] not in values
    if kind == NOT_KEY:
        return tagk not in tags
    raise ValueError(f"unknown kind {kind}")


def visible(tags: dict, filters, explicit_tags) -> bool:
    if not all(holds(kind, tags, k, set(vs)) for k, kind, vs in filters):
        return False
    if explicit_tags:
        return set(tags) == {k for k, kind, _ in filters if kind != NOT_KEY}
    return True


def group_ids(tag_rows, tag_query):
    """(ids, keys): the id of every series -- GROUP_EXCLUDED when a filter fails, GROUP_NONE when it
    is visible but lacks a group-by tag, else the rank of its key -- and the distinct complete
    keys, ascending: tuples of ints compare as the concatenated big-endian uids do."""
    filters, group_by, explicit = parts(tag_query)
    filters = [(k, kind, set(vs)) for k, kind, vs in filters]
    key_of = []
    for row in tag_rows:
        tags = dict(row)
        if not visible(tags, filters, explicit):
            key_of.append(GROUP_EXCLUDED)
        elif all(k in tags for k in group_by):
            key_of.append(tuple(tags[k] for k in group_by))
        else:
            key_of.append(GROUP_NONE)
    keys = sorted(set(k for k in key_of if isinstance(k, tuple)))
    index = {k: i for i, k in enumerate(keys)}
    return [index[k] if isinstance(k, tuple) else k for k in key_of], keys


def counters(ids):
    """(visible, excluded, ungrouped, n_groups) as tsdbhip_tags_info reports them."""
    excluded = sum(1 for i in ids if i == GROUP_EXCLUDED)
    ungrouped = sum(1 for i in ids if i == GROUP_NONE)
    groups = len({i for i in ids if i >= 0})
    return len(ids) - excluded, excluded, ungrouped, groups
