from ._lookup import LookupSampler, as_list


class THGNegativeEdgeSampler(LookupSampler):
    """thgl: keys are (time, source, edge type)."""

    def __init__(self, dataset_name, first_node_id, last_node_id, node_type):
        super().__init__(dataset_name)
        self.first_node_id, self.last_node_id, self.node_type = first_node_id, last_node_id, node_type

    def query_batch(self, pos_src, pos_dst, pos_timestamp, edge_type, split_mode='test'):
        return self._lookup(zip(as_list(pos_timestamp), as_list(pos_src), as_list(edge_type)), split_mode)
