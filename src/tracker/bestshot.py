from .. import _pkg

BestShots = _pkg("bestshot").BestShots
