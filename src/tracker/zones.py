from .. import _pkg

ZoneCounter = _pkg("zones").ZoneCounter
