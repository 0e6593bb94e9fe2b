from .. import _pkg

LeftObjects = _pkg("leftobj").LeftObjects
