from .. import _pkg

HeatMaps = _pkg("heatmap").HeatMaps
