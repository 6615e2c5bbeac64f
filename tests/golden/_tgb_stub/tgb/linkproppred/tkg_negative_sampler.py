from ._lookup import LookupSampler, as_list


class TKGNegativeEdgeSampler(LookupSampler):
    """tkgl: keys are (time, source, edge type)."""

    def __init__(self, dataset_name, first_dst_id, last_dst_id):
        super().__init__(dataset_name)
        self.first_dst_id, self.last_dst_id = first_dst_id, last_dst_id

    def query_batch(self, pos_src, pos_dst, pos_timestamp, edge_type, split_mode='test'):
        return self._lookup(zip(as_list(pos_timestamp), as_list(pos_src), as_list(edge_type)), split_mode)
