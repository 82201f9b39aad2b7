from .blocks import (CHANNEL_MAP, Conv1d, Conv2d, cloud_term_form, cloud_term_route, create_act, create_convblock1d, create_convblock2d,
                     create_norm, expand_cloud_channels, feature_propagation_first_block, fused_first_block, fused_first_conv,
                     fused_local_aggregation, run_convblocks)
from .knn import knn_point, KNN, DenseDilated, DilatedKNN
from .group import (ball_query, create_grouper, gather_operation, get_aggregation_feautres,
                    grouping_operation, torch_grouping_operation, QueryAndGroup, GroupAll, KNNGroup)
from .subsample import fps, furthest_point_sample, random_sample
from .upsampling import three_interpolate, three_interpolation, three_nn
from .local_aggregation import ASSA, ConvPool, LocalAggregation
from .graph_conv import MRConv, EdgeConv, GraphConv, DynConv, ResDynBlock, DenseDynBlock
