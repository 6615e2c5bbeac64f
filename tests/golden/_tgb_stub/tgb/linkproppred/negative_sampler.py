from ._lookup import LookupSampler, as_list


class NegativeEdgeSampler(LookupSampler):
    """tgbl: keys are (source, destination, time)."""

    def query_batch(self, pos_src, pos_dst, pos_timestamp, edge_type=None, split_mode='test'):
        return self._lookup(zip(as_list(pos_src), as_list(pos_dst), as_list(pos_timestamp)), split_mode)
