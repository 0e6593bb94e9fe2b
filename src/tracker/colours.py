from .. import _pkg

TrackColours = _pkg("colours").TrackColours
