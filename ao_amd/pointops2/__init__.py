"""pointops2-style spellings (libs/pointops2/functions/pointops.py:15-55,963-1001,1023-1192) of the
same HIP ops: the six base ops the two libraries share, and the three Stratified-Transformer operators ST-v1m2
calls (attention_step1_v2, dot_prod_with_idx_v3, attention_step2_with_rel_pos_value_v2: ao_amd/stratified,
DESIGN.md section 14).  The older forms of those three raise NotImplementedError naming themselves."""
from . import pointops  # noqa: F401
