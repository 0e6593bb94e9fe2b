from .. import _pkg

Proximity = _pkg("proximity").Proximity
