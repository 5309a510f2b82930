"""Put this directory's parent (`dropin/`) on PYTHONPATH and `import pointgroup_ops` resolves to the MI355X implementation --
pointcept/models/point_group/point_group_v1m1_base.py runs unchanged."""
from ao_amd.pointgroup.ops import ballquery_batch_p, bfs_cluster  # noqa: F401
